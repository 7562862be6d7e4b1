"""A book of vanilla calls in ONE launch (mc_vanilla_book_*) against the five per-call forms of tools/graph_book.py, in one process.

Small options: books of B = 1024 options of 1e4 ... 1e7 paths each (graph_book.py's books: same option, consecutive path ranges),
fp32 and fp64.  Per book, microseconds per option of
    sync calls | async, 1 stream | hipGraph replay | async, 4 contexts | graph, 4 contexts | book run | book launch | book graph
where "book run" is mc_vanilla_book_run_* (synchronous: enqueue, wait, one copy back, closing), "book launch" the asynchronous form
on one stream and "book graph" that launch captured into a hipGraph and replayed.  The forms are timed in alternation, REPS rounds
of every form in turn, and the minimum of each is printed.  Every form's triples are checked against the book's first.
Large entries (--large): a book of 8 x 1.25e7-path entries against one 1e8-path single call, fp32 and fp64, alternated; the
kernel times come from a rocprofv3 run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o book -- python tools/book_speed.py --large --kernels
    python tools/book_speed.py --stats DIR      (per-kernel count and mean duration from the stats file rocprofv3 wrote)
"""
import csv
import glob
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import montecarlocuda_amd as mc  # noqa: E402

VAN = dict(s=100.0, k=100.0, r=0.048790, v=0.2, t=1.0)
SEED = mc.MC_DEFAULT_SEED
B = 1024
REPS = 5


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def small_books(sizes):
    eng = mc.Engine(0)
    eng.set_timing(False)
    engs = [mc.Engine(0) for _ in range(4)]
    names = ["sync calls", "async, 1 stream", "hipGraph replay", "async, 4 contexts", "graph, 4 contexts", "book run", "book launch",
             "book graph"]
    print(f"book of {B} vanilla calls; us per option (paths/s), minimum of {REPS} alternated rounds")
    print(f"{'prec':4s} {'paths/opt':>9s} " + " ".join(f"{n:>21s}" for n in names) + "  best per-call form / best book form")
    for X in ("f32", "f64"):
        struct, _ = eng.prepared("vanilla", X, VAN)
        for n in sizes:
            st = torch.cuda.Stream()
            side = [torch.cuda.Stream() for _ in range(4)]
            structs = [e.prepared("vanilla", X, VAN)[0] for e in engs]
            with torch.cuda.stream(st):
                out = torch.zeros((B, 3), dtype=torch.float64, device="cuda")
                bout = torch.zeros((B, 3), dtype=torch.float64, device="cuda")
            ptrs = [out[i].data_ptr() for i in range(B)]
            firsts = [i * n for i in range(B)]
            entries = eng.book_entries([VAN] * B, n, SEED, firsts, X)
            run_fn = getattr(mc._lib.lib(), f"mc_vanilla_book_run_{X}")
            launch_fn = getattr(mc._lib.lib(), f"mc_vanilla_book_launch_{X}")
            res = (mc._lib.Result * B)()

            def sync_calls():
                for i in range(B):
                    eng.vanilla(VAN, n, SEED, i * n, X)

            def enqueue(stream_of):
                for i in range(B):
                    eng.launch("vanilla", X, struct, SEED, i * n, n, ptrs[i], stream_of(i))

            def async_one():
                enqueue(lambda i: st.cuda_stream)

            def async_four():
                for i in range(B):
                    engs[i & 3].launch("vanilla", X, structs[i & 3], SEED, i * n, n, ptrs[i], side[i & 3].cuda_stream)

            def book_run():
                mc._lib.check(run_fn(eng._ctx, entries, B, res))

            def book_launch(stream=None):
                mc._lib.check(launch_fn(eng._ctx, entries, B, mc._lib.C.c_void_p(bout.data_ptr()),
                                        mc._lib.C.c_void_p(stream if stream is not None else st.cuda_stream)))

            async_one()
            torch.cuda.synchronize()
            want = out.clone()
            book_run()
            got = [(r.sum, r.sum2, float(r.n)) for r in res]
            ref = eng.vanilla(VAN, n, SEED, 5 * n, X)
            assert got[5][2] == ref.n and abs(got[5][0] - ref.sum) <= 3e-6 * abs(ref.sum), (got[5], ref)
            book_launch()
            torch.cuda.synchronize()
            assert [tuple(x) for x in bout.cpu().tolist()] == got, "book launch differs from the book run"
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                enqueue(lambda i: torch.cuda.current_stream().cuda_stream)
            g4 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g4, stream=st):
                cur = torch.cuda.current_stream()
                for s_ in side:
                    s_.wait_stream(cur)
                async_four()
                for s_ in side:
                    cur.wait_stream(s_)
            gb = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gb, stream=st):
                book_launch(torch.cuda.current_stream().cuda_stream)
            bout.zero_()
            gb.replay()
            torch.cuda.synchronize()
            assert [tuple(x) for x in bout.cpu().tolist()] == got, "book graph differs from the book run"
            out.zero_()
            g.replay()
            g4.replay()
            torch.cuda.synchronize()
            assert bool((out == want).all()), "per-call graph forms differ"
            forms = [sync_calls, async_one, g.replay, async_four, g4.replay, book_run, book_launch, gb.replay]
            best = [float("inf")] * len(forms)
            for _ in range(REPS):
                for k, f in enumerate(forms):
                    best[k] = min(best[k], timed(f))
            cells = [f"{t / B * 1e6:8.3f} ({B * n / t:9.3e})" for t in best]
            ratio = min(best[:5]) / min(best[5:])
            print(f"{X:4s} {n:9d} " + " ".join(f"{c:>21s}" for c in cells) + f"  {ratio:8.1f}x", flush=True)
    eng.close()
    for e in engs:
        e.close()


def large(kernels_only=False):
    """8 x 1.25e7-path entries in one book against one 1e8-path call (kernel times: rocprofv3 --stats of this run)."""
    eng = mc.Engine(0)
    for X in ("f32", "f64"):
        book = eng.book_entries([VAN] * 8, 12_500_000, SEED, [i * 12_500_000 for i in range(8)], X)
        res = (mc._lib.Result * 8)()
        run_fn = getattr(mc._lib.lib(), f"mc_vanilla_book_run_{X}")
        best_b = best_s = float("inf")
        for _ in range(20 if kernels_only else 10):
            mc._lib.check(run_fn(eng._ctx, book, 8, res))
            best_b = min(best_b, min(r.kernel_ms for r in res))
            one = eng.vanilla(VAN, 10 ** 8, SEED, 0, X)
            best_s = min(best_s, one.kernel_ms)
        tot = sum(r.sum for r in res)
        print(f"{X}: 8 x 1.25e7 book {best_b * 1e3:.1f} us (events), one 1e8 call {best_s * 1e3:.1f} us (events); "
              f"sums {tot:.6e} vs {one.sum:.6e}", flush=True)
    eng.close()


def stats(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    assert files, f"no kernel_stats.csv under {d}"
    print("kernel (rocprofv3 --kernel-trace --stats): calls, mean us, min us")
    for row in csv.DictReader(open(files[0])):
        name = row["Name"]
        if "vanilla" in name:
            print(f"  {int(row['Calls']):5d} {float(row['AverageNs']) / 1e3:10.1f} {float(row['MinNs']) / 1e3:10.1f}  {name[:110]}")


if __name__ == "__main__":
    if "--stats" in sys.argv:
        stats(sys.argv[sys.argv.index("--stats") + 1])
    elif "--large" in sys.argv:
        large("--kernels" in sys.argv)
    else:
        small_books([10 ** 4, 10 ** 5, 10 ** 6, 10 ** 7] if "--all" in sys.argv or len(sys.argv) == 1 else [int(x) for x in sys.argv[1:]])
