"""The blocked fp32 vanilla kernel without a GPU (csrc/mc_rng.hpp: PhiloxBlock8, csrc/mc_kernels.hpp: vanilla_f32_blocked_kernel,
csrc/mc_launch_shape.hpp: vanilla_blocking):

  * the identity the loop rests on -- eight consecutive units share round 1 and the multiply of round 2 -- word for word
    against the oracle's Philox4x32-10;
  * the instruction counts of the loop hipcc emits (the point of the blocked form is instructions per path: a compiler that
    re-associates the shared product away, spills, or takes a 65th register undoes it silently);
  * the rule that splits a segment between blocks and unit-strided units, as a pure host function.

The last two need hipcc only (like the host-function tests of test_host_logic.py); nothing is launched."""
import collections
import os
import random
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "montecarlocuda_amd", "csrc")
CHECK = os.path.join(ROOT, "tests", "cpp", "vanilla_blocked_check.hip")
M0, M1, W0, W1, MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


# ---- the identity ---------------------------------------------------------------------------------------------------------
def rounds(c, k0, k1, first, count):
    """rounds first .. first + count - 1 (0-based) of Philox4x32-10 on counter c"""
    c0, c1, c2, c3 = c
    for r in range(first, first + count):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ ((k0 + r * W0) & MASK), p1 & MASK, (p0 >> 32) ^ c3 ^ ((k1 + r * W1) & MASK), p0 & MASK
    return [c0, c1, c2, c3]


def block8(unit_hi, base, block, domain, k0, k1):
    """PhiloxBlock8 restated: {global unit: words} of the 8 units at `base` (base % 8 == 0)"""
    p0, p1 = M0 * unit_hi, M1 * block                                   # round 1: both multiplies wave-uniform
    K = (p1 >> 32) ^ k0                                                 # round 1's word 0 is K ^ unit_lo
    c1, c2, c3 = p1 & MASK, (p0 >> 32) ^ domain ^ k1, p0 & MASK
    shared = M0 * ((K & ~7 & MASK) ^ base)                              # PhiloxBlock8::shared
    out = {}
    for l in range(8):
        q0 = shared + M0 * l                                            # the v_mad_u64_u32 with the 64-bit addend
        assert q0 < 1 << 64
        q1 = M1 * c2
        r2 = [(q1 >> 32) ^ c1 ^ ((k0 + W0) & MASK), q1 & MASK, (q0 >> 32) ^ c3 ^ ((k1 + W1) & MASK), q0 & MASK]
        out[base + (l ^ (K & 7))] = rounds(r2, k0, k1, 2, 8)
    return out


def test_plain_python_philox_is_the_oracles(po):
    """the restatement above, all ten rounds, is the oracle's generator and reproduces the known-answer vectors"""
    from conftest import load_golden
    rng = random.Random(5)
    for _ in range(200):
        c, k = [rng.getrandbits(32) for _ in range(4)], [rng.getrandbits(32) for _ in range(2)]
        assert rounds(c, k[0], k[1], 0, 10) == po.philox(c, k)
    cases = load_golden("philox_kat.json")["cases"]
    assert cases
    for case in cases:
        c, k, out = ([int(v, 16) for v in case[f]] for f in ("ctr", "key", "out"))
        assert rounds(c, k[0], k[1], 0, 10) == out == po.philox(c, k)


def test_block_of_8_units_equals_plain_philox(po):
    """A few thousand random (seed, unit_hi, base, block, domain), the edge bases 0, 8 and 2^32 - 8 among them: the block's
    eight word quadruples are those of the oracle's Philox on the engine's counter layout, and they cover base .. base + 7."""
    rng = random.Random(1)
    for t in range(3000):
        hi, blk = rng.getrandbits(32), rng.choice([0, 0, 1, 63, rng.getrandbits(32)])
        dom, k0, k1 = rng.choice([1, 2, 3]), rng.getrandbits(32), rng.getrandbits(32)
        base = [0, 8, (1 << 32) - 8][t % 3] if t < 600 else rng.getrandbits(32) & ~7
        if t % 7 == 0:
            hi = 0
        got = block8(hi, base, blk, dom, k0, k1)
        assert sorted(got) == list(range(base, base + 8))
        for unit, words in got.items():
            assert words == po.philox(po.counter((hi << 32) | unit, blk, dom), [k0, k1]), (t, unit)


# ---- the instruction stream -----------------------------------------------------------------------------------------------
def hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        pytest.skip("hipcc not found")
    return exe


def hipflags():
    m = re.search(r"^HIPFLAGS \?= (.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M)
    return m.group(1).replace("$(ARCH)", "gfx950").split()


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    d = tmp_path_factory.mktemp("blocked_isa")
    asm, res = d / "check.s", d / "resources.txt"
    with open(res, "w") as err:
        subprocess.check_call([hipcc()] + hipflags() + ["--cuda-device-only", "-S", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", str(asm),
                               CHECK, "-Rpass-analysis=kernel-resource-usage"], stderr=err)
    return open(asm).read(), open(res).read()


def blocked_loop(txt, kernel):
    """opcodes of the loop that holds the 8-unit block: from its header label to the branch back to it"""
    names = [m for m in re.findall(r"^(_ZN2mc\w+):", txt, re.M) if kernel in m]
    assert len(names) == 1, names
    body = re.search(r"^" + re.escape(names[0]) + r":[^\n]*\n(.*?)s_endpgm", txt, re.S | re.M).group(1).split("\n")
    loops, label, ops = [], None, []
    for line in body:
        t = line.strip()
        m = re.match(r"^\.L(BB\d+_\d+):", t)
        if m:
            label, ops = m.group(1), []
            continue
        if not t or t.startswith((";", ".")) or label is None:
            continue
        ops.append(t.split()[0])
        if t.startswith("s_cbranch") and t.split()[-1] == ".L" + label:
            loops.append(ops)
            label = None
    big = [o for o in loops if sum(1 for x in o if x.startswith("v_mad_u64_u32")) >= 100]
    assert len(big) == 1, [len(o) for o in loops]
    return big[0]


def resources(res, kernel):
    for b in re.split(r"remark: [^\n]*Function Name: ", res)[1:]:
        if kernel in b.split()[0]:
            return {k: int(re.search(p + r": (\d+)", b).group(1)) for k, p in
                    (("vgpr", "VGPRs"), ("scratch", r"ScratchSize \[bytes/lane\]"), ("occ", r"Occupancy \[waves/SIMD\]"), ("lds", r"LDS Size \[bytes/block\]"))}
    raise AssertionError(kernel)


PLAIN, ANTI = "vanilla_f32_blocked_kernelILb0EEE", "vanilla_f32_blocked_kernelILb1EEE"


def test_blocked_loop_instruction_counts(listing):
    """Per 8 units (32 paths) of the plain estimator: at most 484 VALU instructions (the unit-strided loop: 500), exactly 128
    v_mad_u64_u32 (8 x 15 for rounds 3-10, 7 with the addend, 1 shared), at most 8 x 17 + 1 xors, one add on the counter."""
    txt, _ = listing
    c = collections.Counter(blocked_loop(txt, PLAIN))
    valu = sum(v for k, v in c.items() if k.startswith("v_"))
    xors = sum(v for k, v in c.items() if k.startswith(("v_bitop3_b32", "v_xor_b32")))
    adds = sum(v for k, v in c.items() if re.match(r"v_(add|sub|subrev)_(u32|co_u32|i32)|v_add3_u32|v_lshl_add_u32|v_add_lshl_u32", k))
    mads = sum(v for k, v in c.items() if k.startswith("v_mad_u64_u32"))
    trans = sum(v for k, v in c.items() if re.match(r"v_(exp|log|sin|cos|sqrt)_f32", k))
    print(f"blocked loop, plain: {valu} VALU per 8 units, {mads} v_mad_u64_u32, {xors} xors, {adds} integer adds, {trans} transcendentals, "
          f"{c['s_nop']} s_nop")
    assert valu <= 484
    assert mads == 128
    assert xors <= 8 * 17 + 1
    assert adds == 1
    assert trans == 8 * 12
    assert not any(k.startswith(("scratch_", "buffer_", "global_", "flat_", "ds_")) for k in c), "the loop touches no memory"


def test_blocked_loop_antithetic_counts(listing):
    """the antithetic loop shares the generator's counts; it adds per unit two exponential pairs and their payoffs"""
    txt, _ = listing
    c = collections.Counter(blocked_loop(txt, ANTI))
    assert sum(v for k, v in c.items() if k.startswith("v_mad_u64_u32")) == 128
    assert sum(v for k, v in c.items() if k.startswith(("v_bitop3_b32", "v_xor_b32"))) <= 8 * 17 + 1
    assert sum(v for k, v in c.items() if re.match(r"v_(exp|log|sin|cos|sqrt)_f32", k)) == 8 * 16
    assert not any(k.startswith(("scratch_", "buffer_", "global_", "flat_", "ds_")) for k in c)


@pytest.mark.parametrize("kernel", [PLAIN, ANTI])
def test_blocked_kernel_keeps_8_waves_per_simd(listing, kernel):
    _, res = listing
    r = resources(res, kernel)
    print(kernel, r)
    assert r["scratch"] == 0 and r["vgpr"] <= 64 and r["occ"] == 8
    assert r["lds"] <= 264   # the workgroup reduction's, as before


def test_addend_multiplies_survive_the_compiler(listing):
    """seven multiplies per block take the shared product as their 64-bit addend and the unit's number as an inline constant"""
    txt, _ = listing
    for kernel in (PLAIN, ANTI):
        name = [m for m in re.findall(r"^(_ZN2mc\w+):", txt, re.M) if kernel in m][0]
        body = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)s_endpgm", txt, re.S | re.M).group(1)
        with_addend = re.findall(r"v_mad_u64_u32 v\[\d+:\d+\], s\[\d+:\d+\], s\d+, ([1-7]), v\[\d+:\d+\]", body)
        assert sorted(with_addend) == sorted("1234567" * 2), with_addend   # the loop and the peeled block of the partial sweep


# ---- the split of a segment -----------------------------------------------------------------------------------------------
def split(exe, cases):
    argv = [str(x) for k in cases for x in k]
    out = subprocess.run([str(exe)] + argv, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = {}
    for ln in out.stdout.splitlines():
        a, b = ln.split("->")
        got[tuple(int(x) for x in a.split())] = tuple(int(x) for x in b.split())
    return got


def test_vanilla_blocking_rule(tmp_path):
    """(unit_lo, n_units, stride) -> (head, full sweeps, blocks of a partial sweep, blocked units, unit-strided full trips)"""
    exe = tmp_path / "vanilla_blocked_check"
    subprocess.check_call([hipcc(), "-O1", "-std=c++17", "--offload-arch=gfx950", "-I", CSRC, "-I", os.path.join(ROOT, "include"), CHECK, "-o", str(exe)])
    S = 2048 * 256   # the default grid
    none = (0, 0, 0, 0, 0)
    cases = {
        (0, 25_000_000, S): (0, 5, 25_000_000 // 8 - 5 * S, 25_000_000, 0),   # the 1e8-path call: 5 sweeps + 96 % of a sixth, all blocked
        (0, 5, S): none,                                                   # fewer than 8 units
        (3, 4, S): none,
        (0, 7 * S, S): none,                                               # small calls: the unit-strided kernel, as before
        (0, 8 * S - 1, S): none,                                           # one unit short of a sweep
        (0, 8 * S, S): (0, 1, 0, 8 * S, 0),                                # exactly one block per lane
        (0, 8 * S + 1, S): (0, 1, 0, 8 * S, 0),                            # one unit more: that unit is unit-strided
        (0, 8 * S + 64, S): (0, 1, 0, 8 * S, 0),                           # just past a sweep: no lane takes a straggling block
        (0, 15 * S, S): (0, 1, 0, 8 * S, 7),                               # 7 strides left: 7 unit-strided trips
        (0, 15 * S + S // 2, S): (0, 1, 0, 8 * S, 7),                      # 7.5 strides left: still unit-strided
        (0, 15 * S + S // 2 + 8, S): (0, 1, 15 * S // 16 + 1, 15 * S + S // 2 + 8, 0),   # more: a partial sweep
        (5, 8 * 4096 + 3 + 2, 4096): (3, 1, 0, 8 * 4096, 0),               # a start off the 8-unit grid
        ((1 << 32) - 8 * 1024 * 3, 8 * 1024 * 3, 1024): (0, 3, 0, 8 * 1024 * 3, 0),   # a segment that ends at 2^32 units
        (8, 1 << 31, 311 * 256): (0, (1 << 28) // (311 * 256), 0, (1 << 28) // (311 * 256) * 8 * 311 * 256,
                                  ((1 << 31) - (1 << 28) // (311 * 256) * 8 * 311 * 256) // (311 * 256)),
    }
    rng = random.Random(3)
    rand = []
    for _ in range(400):
        stride = 256 * rng.choice([1, 2, 7, 16, 311, 2048])
        n = rng.choice([rng.randrange(1, 64), rng.randrange(1, 20 * stride), rng.randrange(1, 1 << 31)])
        lo = rng.choice([0, rng.randrange(0, 1 << 20), (1 << 32) - n - rng.randrange(0, 9)])
        if lo >= 0 and lo + n <= 1 << 32:
            rand.append((lo, n, stride))
    got = split(exe, list(cases) + rand)
    assert {k: got[k] for k in cases} == cases
    for (lo, n, stride) in rand:
        head, sweeps, extra, blocked, rest_trips = got[(lo, n, stride)]
        if not blocked:
            assert (head, sweeps, extra, rest_trips) == (0, 0, 0, 0) and (n - min((-lo) % 8, n)) // 8 < stride   # less than one full sweep
            continue
        assert head == (-lo) % 8 and sweeps >= 1 and blocked == 8 * (sweeps * stride + extra) and head + blocked <= n and extra < stride
        assert (lo + head) % 8 == 0
        rest = n - blocked
        assert rest_trips == (rest - head) // stride
        # the unit-strided rest is one flush group of the fp32 partials: at most 7 trips and a partial one = 16 values per accumulator
        assert rest - head < 8 * stride and (not extra or rest < 15)
        # trips of the whole grid, in unit-trips: never more than the unit-strided loop alone takes (+ 1 where a partial sweep
        # leaves up to 14 units over, which the last lanes take)
        trips = 8 * sweeps + (8 if extra else 0) + (0 if extra and extra + rest <= stride else -(-rest // stride))
        assert trips <= -(-n // stride) + (1 if extra else 0), (lo, n, stride)
    # at least 95 % of the 1e8-path call's units run blocked (here: all)
    assert got[(0, 25_000_000, S)][3] >= 0.95 * 25_000_000
