"""pytest configuration: markers, paths, and the golden-fixture loader."""
import json
import os
import sys

import pytest

# This image carries two ROCm runtimes with the same sonames (/opt/rocm and the copy bundled in torch/lib).
# Whichever libamdhip64 is loaded first serves the whole process; torch only finds the device through its
# own copy, so tests that use torch next to libmc_mi355x.so need torch loaded first.
try:
    import torch  # noqa: F401
except ImportError:
    pass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with `-m gpu` on the GPU box)")


def load_golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def fromhex(h):
    return float.fromhex(h)


@pytest.fixture(scope="session")
def po():
    """The CPU oracle bindings (test infrastructure)."""
    from oracle import pyoracle
    pyoracle.build()
    return pyoracle


# ---- the compiled reference (oracle/_ref), live or recorded ----------------------------------------------------------------
# oracle/_ref is built only where the reference sources are mounted.  Its answers to every call the tests make are recorded in
# tests/golden/ref_live.json, so those tests run everywhere: on the recording where the build is absent; where it is present, live
# and checked against the recording.  `MC_RECORD_REF=1 python -m pytest tests -m "not gpu"` (with oracle/_ref built) rewrites it.
REF_LIVE = os.path.join(GOLDEN, "ref_live.json")
RECORD_REF = os.environ.get("MC_RECORD_REF") == "1"


def _hexed(x):
    """JSON form of call arguments and answers: floats as C99 hex (exact), containers element by element."""
    import numpy as np
    if isinstance(x, (float, np.floating)):
        return float(x).hex()
    if isinstance(x, np.ndarray):
        return _hexed(x.tolist())
    if isinstance(x, dict):
        return {k: _hexed(v) for k, v in sorted(x.items())}
    if isinstance(x, (list, tuple)):
        return [_hexed(v) for v in x]
    return x


def _unhexed(x):
    if isinstance(x, str):
        return float.fromhex(x)
    if isinstance(x, list):
        return [_unhexed(v) for v in x]
    return x


class _ReferenceCalls:
    """po.Ref's calls for one (precision, N, build): answered by the live library and/or the recording."""

    def __init__(self, po, store, X, n, opt):
        self.po, self.store, self.X, self.n, self.opt = po, store, X, n, opt
        self.live = po.Ref(X, n, opt) if po.ref_available(X, n, opt) else None

    def _call(self, method, *args):
        import numpy as np
        key = json.dumps([self.X, self.n, self.opt, method, _hexed(args)])
        if self.live is None:
            assert key in self.store["calls"], f"no recorded answer of the compiled reference to {key}"
            got = _unhexed(self.store["calls"][key])
        else:
            got = _hexed(getattr(self.live, method)(*args))
            if RECORD_REF:
                self.store["calls"][key] = got
            else:
                assert self.store["calls"].get(key) == got, f"the compiled reference no longer answers {key} as recorded"
            got = _unhexed(got)
        if method == "chol":
            return np.array(got, dtype=self.po.NP[self.X])
        return tuple(got)

    def vanilla(self, o, paths, seed):
        return self._call("vanilla", o, paths, seed)

    def basket(self, b, paths, seed):
        return self._call("basket", b, paths, seed)

    def cva(self, c, paths, seed):
        return self._call("cva", c, paths, seed)

    def chol(self, c):
        return self._call("chol", c)


@pytest.fixture(scope="session")
def ref(po):
    """ref(X, n=3, opt="") -> the compiled reference's host path (vanilla / basket / cva / chol), live or recorded."""
    store = {"calls": {}}
    if not RECORD_REF:
        with open(REF_LIVE) as f:
            store = json.load(f)
    yield lambda X, n=3, opt="": _ReferenceCalls(po, store, X, n, opt)
    if RECORD_REF:
        store["meta"] = {"source": "oracle/_ref: the reference's MonteCarloHost.c compiled unmodified by oracle/Makefile",
                         "key": "[precision, N, build, method, arguments]; floats as C99 hex",
                         "regenerate": "MC_RECORD_REF=1 python -m pytest tests -m 'not gpu', with oracle/_ref built"}
        with open(REF_LIVE, "w") as f:
            json.dump({"meta": store["meta"], "calls": dict(sorted(store["calls"].items()))}, f, indent=0)
            f.write("\n")

