"""A book of vanilla calls in one launch (mc_vanilla_book_*, Engine.vanilla_book): against the single calls on the same inputs,
against a float64 reference on the kernels' own normals, the bit-for-bit rules of include/mc_mi355x.h, the edges (the 2^32-unit seam,
65 536 entries, one 1e9-path entry among tiny ones), the launch form and its hipGraph capture, alternation with other products on one
context, the refusals and the C driver drivers/bookOpt."""
import math
import os
import random
import subprocess

import numpy as np
import pytest

import greeks_ref as gr
from test_gpu_parity import SEED, TOL, VAN, BS_EXACT, CVA0, basket_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPB = {"f32": 4, "f64": 8}
U32 = 1 << 32
REL = {"f32": 3e-6, "f64": 1e-12}   # the sums: summation order only (fp32: partial sums of at most 8 trips x 4 payoffs)


@pytest.fixture(scope="module")
def mc():
    import montecarlocuda_amd as mc
    return mc


@pytest.fixture(scope="module")
def eng(mc):
    e = mc.Engine(0)
    yield e
    e.close()


def random_book(X, count=300, seed=7, big=True):
    rnd = random.Random(seed)
    npb = NPB[X]
    sizes = [1, 3, npb - 1, npb + 1, 1000, 100_000] + ([1_000_000] if big else [])
    book = []
    for i in range(count):
        o = dict(s=rnd.uniform(60, 140), k=rnd.uniform(50, 150), r=rnd.uniform(0.0, 0.08), v=rnd.uniform(0.05, 0.6), t=rnd.uniform(0.1, 3.0))
        n = sizes[i % len(sizes)]
        first = rnd.randrange(0, 10 ** 7) if i % 3 else 0      # mostly offsets that are not multiples of NPB
        book.append((o, n, rnd.getrandbits(64), first))
    return book


def run_book(e, book, X):
    return e.vanilla_book([b[0] for b in book], [b[1] for b in book], [b[2] for b in book], [b[3] for b in book], X)


def triples(res):
    return [(r.sum, r.sum2, r.n) for r in res]


def close(a, b, rel):
    return abs(a - b) <= rel * max(abs(a), abs(b)) + 1e-300


@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("anti", [False, True])
def test_book_matches_single_calls_and_reference(mc, eng, X, anti):
    """Every entry of a random ~300-entry book against Engine.vanilla on the same option, seed and range (n equal, sums within the
    summation-order bound, expected and confidence from those), and the entries of at most 1e5 paths against the float64 reference
    on Engine.normals (the bound on a sum is the sum of the per-path bounds)."""
    eng.set_antithetic(anti)
    try:
        book = random_book(X, seed=11 + anti)
        res = run_book(eng, book, X)
        for (o, n, seed, first), r in zip(book, res):
            one = eng.vanilla(o, n, seed, first, X)
            assert r.n == one.n == n
            assert close(r.sum, one.sum, REL[X]) and close(r.sum2, one.sum2, 2 * REL[X]), (o, n, first, r, one)
            rt = [float(np.float32(o[c])) if X == "f32" else o[c] for c in "rt"]    # the discount of the entry's own option struct
            e, c = mc.closing(r.sum, r.sum2, n, math.exp(-rt[0] * rt[1]))
            assert r.expected == e and (r.confidence == c or (math.isnan(c) and math.isnan(r.confidence)))   # n = 1: no interval
            assert close(r.expected, one.expected, 2 * REL[X])   # (the interval of a few paths is ill-conditioned: checked through closing)
            if n <= 100_000:
                draw = lambda domain, u0, m, block: eng.normals(seed, domain, u0, m, block, X)
                z = gr.vanilla_normals(draw, first, n, NPB[X])
                p = gr.vanilla(o, z)
                val, b = p.value[0], TOL[X]["pay"] * p.scale[0]
                if anti:
                    m = gr.vanilla(o, -z)
                    val, b = 0.5 * (val + m.value[0]), 0.5 * (b + TOL[X]["pay"] * m.scale[0])
                assert abs(r.sum - val.sum()) <= b.sum() + 1e-9, (o, n, first)
                assert abs(r.sum2 - (val * val).sum()) <= (2 * np.abs(val) * b + b * b).sum() + 1e-9, (o, n, first)
    finally:
        eng.set_antithetic(False)


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_bit_for_bit_rules(mc, eng, X):
    """The same entry gives the same triple (==) at index 0 and 4000, in a book of 1 and of 5000, in a shuffled book, on contexts with
    other `blocks`, on a repeat call, and in the fused and the two-launch finish."""
    probe = random_book(X, count=40, seed=5)
    filler = random_book(X, count=5000, seed=6, big=False)
    alone = [triples(run_book(eng, [p], X))[0] for p in probe]
    for k, p in enumerate(probe[:8]):
        at0 = triples(run_book(eng, [p] + filler[1:], X))[0]
        at4000 = triples(run_book(eng, filler[:4000] + [p] + filler[4001:], X))[4000]
        assert at0 == alone[k] == at4000, k
    whole = triples(run_book(eng, probe, X))
    assert whole == alone
    assert triples(run_book(eng, probe, X)) == whole            # repeat call
    order = list(range(len(probe)))
    random.Random(3).shuffle(order)
    shuffled = triples(run_book(eng, [probe[i] for i in order], X))
    assert [shuffled[order.index(i)] for i in range(len(probe))] == whole
    eng.set_finish(False)
    try:
        assert triples(run_book(eng, probe, X)) == whole
    finally:
        eng.set_finish(True)
    for blocks in (1, 7, 3000):
        with mc.Engine(0, blocks) as e:
            assert triples(run_book(e, probe, X)) == whole, blocks


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_seam_and_many_entries(mc, eng, X):
    """An entry across the 2^32-unit seam against the single call and the reference; 65 536 entries of 1e3 paths: every n right and
    no triple left poisoned (the run form checks n), prices near Black-Scholes on average."""
    npb = NPB[X]
    first = U32 * npb - 3 * 256 * npb - 5
    n = 6 * 256 * npb + 11
    r = eng.vanilla_book([VAN], n, SEED, first, X)[0]
    one = eng.vanilla(VAN, n, SEED, first, X)
    assert r.n == n and close(r.sum, one.sum, REL[X]) and close(r.sum2, one.sum2, 2 * REL[X])
    z = gr.vanilla_normals(lambda d, u0, m, b: eng.normals(SEED, d, u0, m, b, X), first, n, npb)
    p = gr.vanilla(VAN, z)
    assert abs(r.sum - p.value[0].sum()) <= (TOL[X]["pay"] * p.scale[0]).sum() + 1e-9
    B = 65536
    res = eng.vanilla_book([VAN] * B, 1000, list(range(B)), 0, X)
    assert all(x.n == 1000 for x in res)
    mean = sum(x.expected for x in res) / B
    assert abs(mean - BS_EXACT) < 3.5 * 15.0 / math.sqrt(1000.0 * B)


def test_large_entry_among_tiny_ones(mc, eng):
    """One 1e9-path fp32 entry among 1000 tiny ones: equal to the single call within the summation-order bound, and to Black-Scholes
    within its confidence interval."""
    tiny = [(VAN, 1 + i % 7, 1000 + i, i) for i in range(1000)]
    book = tiny[:500] + [(VAN, 10 ** 9, SEED, 12345)] + tiny[500:]
    res = run_book(eng, book, "f32")
    big = res[500]
    one = eng.vanilla(VAN, 10 ** 9, SEED, 12345, "f32")
    assert big.n == 10 ** 9 and close(big.sum, one.sum, REL["f32"]) and close(big.sum2, one.sum2, 2 * REL["f32"])
    assert abs(big.expected - BS_EXACT) < 3.5 / 1.96 * big.confidence + 2e-5
    for (o, n, seed, first), r in zip(tiny, res[:500] + res[501:]):
        assert r.n == n


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_launch_form_and_graph_capture(mc, eng, X):
    """vanilla_book_launch into device memory gives the run form's bits; a hipGraph capture of it (tables resident), replayed twice,
    gives the same bits both times."""
    torch = pytest.importorskip("torch")
    book = random_book(X, count=64, seed=9, big=False)
    want = triples(run_book(eng, book, X))
    args = ([b[0] for b in book], [b[1] for b in book])
    kw = dict(seeds=[b[2] for b in book], first_paths=[b[3] for b in book], precision=X)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        out = torch.zeros((len(book), 3), dtype=torch.float64, device="cuda")
        eng.vanilla_book_launch(*args, out.data_ptr(), stream=st.cuda_stream, **kw)
        torch.cuda.synchronize()
        assert [tuple(x) for x in out.cpu().tolist()] == [(s, q, float(n)) for s, q, n in want]
        out.zero_()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            eng.vanilla_book_launch(*args, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream, **kw)
        for _ in range(2):
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert [tuple(x) for x in out.cpu().tolist()] == [(s, q, float(n)) for s, q, n in want]


def test_alternation_with_other_products(mc, eng):
    """On one context: book, single vanilla, basket n = 17 (a constant table of its own), CVA (the per-date table), book again, twice
    over -- every result equal to the same call on a fresh context of its own.  A repeated identical book uploads nothing: its
    table_upload_ms is 0 when it follows itself and when a basket or CVA call came in between."""
    book = random_book("f64", count=50, seed=13, big=False)
    b17 = basket_inputs(mc, 17, "f64")
    cva = dict(CVA0, n_grid=64)
    calls = [lambda e: triples(run_book(e, book, "f64")), lambda e: eng_sum(e.vanilla(VAN, 100003, SEED, 7, "f64")),
             lambda e: eng_sum(e.basket(b17, 50001, SEED, 3, "f64")), lambda e: eng_sum(e.cva(cva, 20001, SEED, 0, "f64"))]
    alone = []
    for f in calls:
        with mc.Engine(0) as fresh:
            alone.append(f(fresh))
    for _ in range(2):
        for k, f in enumerate(calls):
            assert f(eng) == alone[k], k
            if k == 0:
                assert triples(run_book(eng, book, "f64")) == alone[0]
                assert eng.last_call_stats()["table_upload_ms"] == 0.0
    assert triples(run_book(eng, book, "f64")) == alone[0]
    assert eng.last_call_stats()["table_upload_ms"] == 0.0     # after the CVA call: the book's tables are still resident


def eng_sum(r):
    return (r.sum, r.sum2, r.n)


def test_refusals(mc, eng):
    """Each refusal of include/mc_mi355x.h returns its code and names the first bad entry; the next call on the context succeeds."""
    good = [(VAN, 1000, SEED, 0)] * 5
    ok = triples(run_book(eng, good, "f64"))
    bad = {"n_paths == 0": (VAN, 0, SEED, 0), "overflows": (VAN, 10, SEED, 2 ** 64 - 5),
           "more than 8 segments": (VAN, 9 * 2 ** 31 * 8, SEED, 0), "need s>0": (dict(VAN, s=-1.0), 10, SEED, 0),
           "outside the range of a double": (dict(VAN, v=400.0, t=100.0), 10, SEED, 0)}
    for why, entry in bad.items():
        for X in ("f32", "f64"):
            if why == "outside the range of a double" and X == "f32":
                entry = (dict(VAN, v=60.0, t=100.0), 10, SEED, 0)
            with pytest.raises(mc._lib.McError) as ex:
                run_book(eng, good[:3] + [entry] + good[:1] + [entry], X)
            assert "mc error 1" in str(ex.value) and "entry 3" in str(ex.value), (why, X, str(ex.value))
            assert triples(run_book(eng, good, "f64")) == ok
    for count in (0, mc._lib.MAX_BOOK + 1):
        arr = eng.book_entries([VAN], 10)
        rc = mc._lib.lib().mc_vanilla_book_run_f64(eng._ctx, arr, count, (mc._lib.Result * 1)())
        assert rc == 1 and "count" in mc._lib.lib().mc_last_error().decode()
    for setup, X in ((lambda: eng.set_generator("xorwow"), "f64"), (lambda: eng.set_generator("xorwow"), "f32"),
                     (lambda: eng.set_normals("f32"), "f64")):
        setup()
        try:
            with pytest.raises(mc._lib.McError) as ex:
                run_book(eng, good, X)
            assert "mc error 4" in str(ex.value)
        finally:
            eng.set_generator("philox")
            eng.set_normals("native")
    assert triples(run_book(eng, good, "f64")) == ok
    s = eng.last_call_stats()
    assert s["wall_ms"] > 0


def test_c_driver_matches_python(mc, eng):
    """drivers/bookOpt prices a strike x maturity grid in one book call; its prices equal Engine.vanilla_book's on the same entries."""
    exe = os.path.join(ROOT, "drivers", "bookOpt")
    assert os.path.exists(exe), "drivers/bookOpt not built (build())"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("K=")]
    assert len(rows) >= 12
    opts, prices = [], []
    for r in rows:
        kv = dict(x.split("=") for x in r if "=" in x)
        opts.append(dict(s=100.0, k=float(kv["K"]), r=0.05, v=0.2, t=float(kv["T"])))
        prices.append(float(kv["price"]))
    n = int(out.stdout.split("paths=")[1].split()[0])
    res = eng.vanilla_book(opts, n, SEED, 0, "f64")
    for p, r in zip(prices, res):
        assert abs(p - r.expected) <= 1e-9 * max(1.0, abs(p))
