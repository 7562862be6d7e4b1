"""Float64 model of the CVA PRICING kernels (not a test module): cva_kernel, cva_dates_kernel and cva_split_kernel
(csrc/mc_kernels.hpp), the cut between them (csrc/mc_launch_shape.hpp: cva_plan; csrc/mc_api.hip: cva_enqueue).

`price` is greeks_ref.cva's own CVA (value[0], scale[0]) -- the independent float64 model the Greeks tests hold
cva_greeks_kernel to -- as a one-row `Paths`, with the antithetic pair mean.  The exposure (S - K)^+ is continuous, so the intrinsic
date has no jump term; the only one is the 1e-9 step of the Hastings cnd itself at d = 0, on paths with a d1 or d2 within eps of 0
(`price`).  The per-path bound is greeks_ref.bound(p, TOL[X]["pay"]): the eps the Greeks tests use for this plane, unchanged.

`schedule` classifies a (t, n_grid) in a precision: how the grid ends (full, cut, intrinsic), the parity of n_bs and where the
last date sits inside the date-parallel form's chunks and rounds.  `lanes_model` evaluates the same float64 formulas organised as
cva_dates_role organises them (rounds of 8 L dates, chunks of 8 dates per lane, date pairs, table rows per date) so that the index
errors of MUTATIONS can be stated in it; test_cva_ref.py shows that it is `price` when nothing is mutated and that every mutation
moves almost every path of the GPU test's markets beyond the fp32 bound.

CASES (schedule cases) and EXTRA (unconstrained markets) are what test_gpu_cva_ref.py runs and test_cva_ref.py guards.
"""
import math
from collections import namedtuple

import numpy as np

import greeks_ref as gr
from test_gpu_parity import TOL

CH = 8                      # CVA_DATES_CH: dates per lane and round
LANES = [1, 2, 4, 8, 16, 32, 64]


# ---- the price ------------------------------------------------------------------------------------------------------
HASTINGS_STEP = abs(1.0 - 2.0 * float(gr.cnd(0.0)))      # 1.0e-9: the model's cnd steps by this much at d = 0 (greeks_ref.py)


def _cnd_steps(c, z, X):
    """Per path: the size of the value's step should every d1 and d2 change side of 0 -- the Hastings cnd is discontinuous there,
    |LGD| sum_j dp_j (S_j + K e^{-r tau_j}) HASTINGS_STEP -- and the distance of the nearest d1 or d2 to 0 in units of its own
    forward-error scale (greeks_ref.cva's ed)."""
    s0, k, r, v = (float(c[q]) for q in "skrv")
    dt, tj, tau, dp = gr.cva_dates(c, X)
    bs = tau > 0
    z = np.asarray(z, dtype=np.float64)[:, :tj.size][:, bs]
    if z.shape[1] == 0:
        return np.zeros(z.shape[0]), np.full(z.shape[0], np.inf)
    tau, dp = tau[bs], dp[bs]
    W = np.cumsum(z, axis=1)
    W_abs = np.cumsum(np.abs(W), axis=1)
    sdt, sig = math.sqrt(dt), v * np.sqrt(tau)
    lns = math.log(s0) + np.arange(1, tau.size + 1) * (r - 0.5 * v * v) * dt + v * sdt * W
    d1 = (lns - math.log(k) + (r + 0.5 * v * v) * tau) / sig
    ed = 1.0 + np.abs(d1) + v * sdt * (np.abs(W) + W_abs) / sig
    jump = abs(float(c["lgd"])) * HASTINGS_STEP * (dp * (np.exp(lns) + k * np.exp(-r * tau))).sum(axis=1)
    return jump, np.minimum(np.abs(d1) / ed, np.abs(d1 - sig) / (ed + sig)).min(axis=1)      # (d2 = d1 - sig: one more rounding of size sig)


def price(c, z, X, anti=False):
    """Paths of shape (1, n): the CVA of every path of normals z (n, >= n_dates), scale in units of the unit roundoff.  The
    exposure (S - K)^+ is continuous: the intrinsic date has no jump.  The one step the price has is the Hastings cnd's own at
    d = 0 (HASTINGS_STEP): a path with a d1 or d2 within eps of 0 at some date -- none among the device's normals in fp64, the
    steered ones of `chosen_normals` -- carries it as its jump, as two correct implementations may land on opposite sides."""
    z = np.asarray(z, dtype=np.float64)
    p = gr.cva(c, z, X)
    value, scale = p.value[:1], p.scale[:1]
    jump, edge = _cnd_steps(c, z, X)
    if anti:
        q = gr.cva(c, -z, X)
        value, scale = 0.5 * (value + q.value[:1]), 0.5 * (scale + q.scale[:1])
        jm, em = _cnd_steps(c, -z, X)
        jump, edge = 0.5 * (jump + jm), np.minimum(edge, em)
    return gr.Paths(value, scale, jump[None, :], edge)


def bound(p, X):
    return gr.bound(p, TOL[X]["pay"])[0]


# ---- schedules ------------------------------------------------------------------------------------------------------
Schedule = namedtuple("Schedule", "n_dates n_bs ending parity chunk_pos")


def schedule(c, X):
    """n_dates, n_bs, ending ("full": every date of the grid, the last with tau > 0; "cut": a date with tau < 0 dropped;
    "intrinsic": the last date has tau == 0), n_bs % 2, and the last date's 0-based position inside its 8-date chunk."""
    tau = gr.cva_dates(c, X)[2]
    n_dates = tau.size
    intrinsic = n_dates > 0 and tau[-1] == 0
    ending = "intrinsic" if intrinsic else ("cut" if n_dates < int(c["n_grid"]) else "full")
    n_bs = n_dates - int(intrinsic)
    return Schedule(n_dates, n_bs, ending, n_bs % 2, (n_dates - 1) % CH)


def lanes_used(forced, n_dates):
    """Lanes per path of a call forced to `forced` lanes (cva_plan): a path cannot use more lanes than it has chunks."""
    max_l = 0
    while max_l < 6 and (CH << max_l) < n_dates:
        max_l += 1
    return 1 << min(int(math.log2(forced)), max_l) if forced > 1 else 1


def round_pos(s, L):
    """The last date's 0-based position inside its round of 8 L dates."""
    return (s.n_dates - 1) % (CH * L)


# ---- the model, organised as the date-parallel kernel ---------------------------------------------------------------
def _running_sums(z, L, mutation):
    """W_j = z_1 + ... + z_j formed as cva_dates_role forms it: the previous rounds' total + the chunks of the lanes below + the
    lane's own dates."""
    n, nd = z.shape
    per = CH * L
    rounds = (nd + per - 1) // per
    zp = np.zeros((n, rounds * per))
    zp[:, :nd] = z
    zp = zp.reshape(n, rounds, L, CH)
    chunk = zp.sum(axis=3)                                   # (n, rounds, L)
    incl = np.cumsum(chunk, axis=2)
    before = incl - chunk                                    # the lanes below
    total = incl[:, :, -1]                                   # (n, rounds)
    done = np.cumsum(total, axis=1) - total                  # the previous rounds
    W = done[:, :, None, None] + before[:, :, :, None] + np.cumsum(zp, axis=3)
    if mutation == "lane_first_date_misses_chunk_below":
        W[:, :, 1:, 0] -= chunk[:, :, :-1]
    if mutation == "second_round_misses_first_total":
        W[:, 1:] -= total[:, :1, None, None]
    return W.reshape(n, rounds * per)[:, :nd]


def lanes_model(c, z, X, lanes=1, anti=False, mutation=None):
    """The CVA of every path, float64, in the date-parallel kernel's organisation with `lanes` lanes per path (as forced:
    lanes_used cuts it to the grid), optionally with one of MUTATIONS."""
    s0, k, r, v, lgd = (float(c[q]) for q in ("s", "k", "r", "v", "lgd"))
    dt, tj, tau, dp = gr.cva_dates(c, X)
    nd = tj.size
    n = np.asarray(z).shape[0]
    if nd == 0:
        return np.zeros(n)
    L = lanes_used(lanes, nd)
    W = _running_sums(np.asarray(z, dtype=np.float64)[:, :nd], L, mutation)
    row = np.arange(nd)                                      # the table row every date reads
    if mutation == "pair_rows_exchanged":
        row = np.where((row ^ 1) < nd, row ^ 1, row)         # (an unpaired last date keeps its own)
    a, bx = (r - 0.5 * v * v) * dt, v * math.sqrt(dt)
    xk = math.log(s0) + (row + 1) * a                        # ln S_j - bx W_j
    xk_intrinsic = xk.copy()
    if mutation == "intrinsic_neighbour_xk" and nd >= 2:
        xk_intrinsic[-1] = xk[-2]
    tau_r, dp_r = tau[row], dp[row]
    bs = tau_r > 0
    sig = v * np.sqrt(np.where(bs, tau_r, 1.0))
    disc = k * np.exp(-r * tau_r)

    def exposures(sign_spot, sign_d):
        lns = xk + bx * sign_spot * W
        d1 = (xk + bx * sign_d * W - math.log(k) + (r + 0.5 * v * v) * tau_r) / sig
        closed = np.exp(lns) * gr.cnd(d1) - disc * gr.cnd(d1 - sig)
        return np.where(bs, closed, np.maximum(np.exp(xk_intrinsic + bx * sign_spot * W) - k, 0.0))

    ee = exposures(1.0, 1.0)
    if anti:
        ee = 0.5 * (ee + exposures(-1.0, 1.0 if mutation == "anti_mirror_spot_only" else -1.0))
    total = (ee * dp_r).sum(axis=1)
    if mutation == "date_beyond_cut_contributes":
        total = total + ee[:, -1] * dp_r[-1]
    return lgd * total


Mutation = namedtuple("Mutation", "endings lanes anti what")
# name -> the schedule endings, forced lane counts and estimators it applies to (and it needs the dates it acts on: `applies`)
MUTATIONS = {
    "intrinsic_neighbour_xk": Mutation(("intrinsic",), LANES, (False, True),
                                       "the intrinsic date priced with the neighbouring date's ln-spot constant"),
    "pair_rows_exchanged": Mutation(("full", "cut", "intrinsic"), LANES, (False, True), "the two dates of every pair exchange their table rows"),
    "lane_first_date_misses_chunk_below": Mutation(("full", "cut", "intrinsic"), LANES[1:], (False, True),
                                                   "a lane's first date misses the sum of the chunk below it"),
    "second_round_misses_first_total": Mutation(("full", "cut", "intrinsic"), LANES[1:], (False, True),
                                                "the second and later rounds miss the first round's total"),
    "date_beyond_cut_contributes": Mutation(("cut",), LANES, (False, True), "a date beyond a cut schedule still contributes, from the last row"),
    "anti_mirror_spot_only": Mutation(("full", "cut", "intrinsic"), LANES, (True,), "the antithetic mirror negates W in the spot but not in d1 / d2"),
}


def applies(name, s, lanes, anti):
    """Whether mutation `name` acts on a schedule s at `lanes` forced lanes under the estimator."""
    m = MUTATIONS[name]
    if s.ending not in m.endings or lanes not in m.lanes or anti not in m.anti or s.n_dates < 2:
        return False
    L = lanes_used(lanes, s.n_dates)
    if name == "lane_first_date_misses_chunk_below":
        return L >= 2                                         # (then the grid has more than one chunk)
    if name == "second_round_misses_first_total":
        return L >= 2 and s.n_dates > CH * L
    return True


# ---- the cases ------------------------------------------------------------------------------------------------------
# (t, n_grid) by how the schedule ends, as test_cva_ref.py checks with `schedule` in both precisions
INTRINSIC_EVEN = [(1.125, 9), (2.125, 17), (8.125, 65), (16.125, 129),    # the intrinsic date starts a chunk (65, 129: a round at L = 8 / 16)
                  (1.375, 11), (1.625, 13)]                               # ... sits mid-chunk
INTRINSIC_ODD = [(0.375, 24), (1.0, 16), (1.0, 64), (1.0, 256)]
CUT = [(1.0, 250), (1.0, 129),            # cut in both precisions
       (1.0, 500), (0.7321, 37),          # cut in fp64 only
       (0.7321, 100)]                     # an exact 0 in fp32 only
FULL = [(1.0, 63), (1.0, 65), (1.0, 127), (2.0, 514)]
CUT_LONG = [(1.0, 258)]                   # 257 dates in both precisions: a cut schedule, and a last pair of one date, at 64 lanes in fp32
CASES = INTRINSIC_EVEN + INTRINSIC_ODD + CUT + FULL + CUT_LONG
# a case whose first seed drew a market on which some mutation that applies moved fewer than 90 % of the paths beyond the fp32
# bound (out of the money at the last date, defint * dt or the step drift too small: test_cva_ref.py): the seed moves on by
# 100 000 per step, the condition stays
RESEEDED = {(1.125, 9): 99, (2.125, 17): 4143, (8.125, 65): 289, (16.125, 129): 525, (1.375, 11): 592, (1.625, 13): 962, (0.375, 24): 4169,
            (1.0, 16): 2394, (1.0, 64): 49, (1.0, 256): 10, (1.0, 250): 108, (1.0, 129): 20, (1.0, 500): 100, (0.7321, 37): 142,
            (0.7321, 100): 151, (1.0, 63): 31, (1.0, 65): 70, (1.0, 127): 27, (2.0, 514): 1200, (1.0, 258): 330}


def seed_of(case):
    return 7000 + CASES.index(case) + 100_000 * RESEEDED.get(case, 0)


def market(case):
    """The market of a schedule case: greeks_ref.random_cva's draw with t and n_grid overwritten (one market for both precisions)."""
    t, n_grid = case
    return dict(gr.random_cva(np.random.default_rng(seed_of(case))), t=t, n_grid=n_grid)


N_EXTRA = 8


def extra_market(X, i):
    """Eight unconstrained markets per precision; 5: lgd < 0, 6: lgd = 0, 7: defint = 0 (the last two price every path at 0)."""
    c = gr.random_cva(np.random.default_rng({"f32": 8100, "f64": 8200}[X] + i))
    if i == 5:
        c["lgd"] = -c["lgd"]
    if i == 6:
        c["lgd"] = 0.0
    if i == 7:
        c["defint"] = 0.0
    return c


def threshold_market(n_grid):
    """t = 2 on the grids either side of cva_enqueue's thresholds (test_gpu_cva_ref.py d, e)."""
    return dict(gr.random_cva(np.random.default_rng(9000 + n_grid)), t=2.0, n_grid=n_grid)


# ---- chosen normals (test_gpu_cva_ref.py g) --------------------------------------------------------------------------
CHOSEN_CASES = [(1.625, 13), (1.0, 129)]       # intrinsic (mid-chunk, even n_bs); cut


def chosen_normals(c, X, rng, n=600):
    """Standard normals (rounded to the precision) with rows steered onto the model's steps: d1 or d2 within a few ulp of 0 at
    some date, the spot at the last date within a few ulp of K, and single normals at the generator's extremes."""
    R = np.float32 if X == "f32" else np.float64
    s0, k, r, v = (float(c[q]) for q in "skrv")
    dt, tj, tau, _ = gr.cva_dates(c, X)
    nd = tj.size
    z = rng.standard_normal((n, nd)).astype(R).astype(np.float64)
    a, bx = (r - 0.5 * v * v) * dt, v * math.sqrt(dt)
    zmax = 6.7 if X == "f32" else 8.5
    row = 0
    for which in ("d1", "d2", "spot"):
        for j in sorted({0, 1, nd // 2, nd - 2, nd - 1} & set(range(nd))):       # 0-based date
            if which == "spot":
                j = nd - 1
                target = math.log(k)
            else:
                if tau[j] <= 0:
                    continue
                sig = v * math.sqrt(tau[j])
                target = math.log(k) - (r + 0.5 * v * v) * tau[j] + (sig * sig if which == "d2" else 0.0)     # ln S_j at which d = 0
            for ulps in (-3, -1, 0, 1, 3):
                before = z[row, :j].sum()
                w = (target - math.log(s0) - (j + 1) * a) / bx - before      # the normal that lands on the step
                if abs(w) < zmax:
                    z[row, j] = float(R(w)) + ulps * float(np.spacing(R(w)))
                row += 1
    for j in sorted({0, 7, 8, nd - 1} & set(range(nd))):
        for sign in (-1.0, 1.0):
            z[row, j] = sign * zmax
            row += 1
    assert row < n
    return z.astype(R)


# host thresholds of cva_enqueue, in dates: the per-date table in 48 KB of LDS (date-parallel) and in 24 KB (split launch)
DATES_MAX = {"f64": 1024, "f32": 2048}
SPLIT_MAX = {"f64": 512, "f32": 1024}
THRESHOLD_GRIDS = {"f64": [(1024, True), (1026, False)], "f32": [(2048, True), (2049, False)]}    # (n_grid, date-parallel possible)
SPLIT_GRIDS = {"f64": [(512, True), (514, False)], "f32": [(1024, True), (1026, False)]}          # (n_grid, split possible)
PAIR_ROW_GRIDS = [682, 683, 684]     # fp32, one lane per path: n_bs; the pair rows fit 16 KB of LDS up to n_bs / 2 = 341
