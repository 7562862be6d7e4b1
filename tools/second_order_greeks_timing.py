"""Kernel times of the second-order Greeks against their first-order siblings (profiles/second_order_greeks_kernel_times.log).

GPU box: rocprofv3 --kernel-trace --stats -d <dir> -o run -- python3 tools/second_order_greeks_timing.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import montecarlocuda_amd as mc
import greeks_ref as gr

o = dict(s=100.0, k=100.0, r=0.048790, v=0.2, t=1.0)
with mc.Engine(0) as e:
    for X in ("f32", "f64"):
        for rep in range(4):
            a = e.vanilla_greeks(o, 10 ** 8, 1, 0, X)
            b = e.vanilla_greeks2(o, 10 ** 8, 1, 0, X)
        print(X, "vanilla_greeks", a[0].kernel_ms, "vanilla_greeks2", b[0].kernel_ms, "gamma", b[3].expected, "+-", b[3].confidence,
              "vanna", b[4].expected, "+-", b[4].confidence, flush=True)
    for na in (4, 16):
        bk = gr.random_basket(np.random.default_rng(na), na, lambda c: mc.chol(c, "f64"))
        for rep in range(3):
            a = e.basket_greeks(bk, 10 ** 7, 1, 0, "f64")
            b = e.basket_gamma(bk, 10 ** 7, 1, 0, "f64")
        print("n", na, "basket_greeks f64", a[0].kernel_ms, "basket_gamma f64", b[0].kernel_ms, flush=True)
