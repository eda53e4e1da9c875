"""k4_round_half_away (csrc/k4_common.h) is written as (int)(x + copysignf(0.49999997f, x)) instead of (int)roundf(x): 3 vector instructions
instead of 7, three times per sample of the geometry kernel.  The two forms must name the same integer for every fp32 value the MaskGrid index
can take.  Checked here in numpy's fp32 arithmetic (IEEE round-to-nearest-even additions, the GPU's): before the float -> int conversion both
forms are fp32 values, and equal fp32 values convert equally, so the comparison is on trunc(x + c) against C round(x).

Cases: every n +- 0.5 with its two fp32 neighbours for |n| < 2^23 (every value at which round() changes, and the values next to it), both
signs, zeros, subnormals, the powers of two 2^23 .. 2^31 with their neighbours, the constant's own neighbourhood, inf and NaN.  The run over
all 2^32 bit patterns (python tests/test_round_identity.py --exhaustive, a few minutes on one thread) is recorded in
profiles/geom_fast_path.md."""
import sys

import numpy as np

HALF_PRED = np.float32(0.49999997)


def c_round(x):
    """C roundf(): halves away from zero, exact in fp32 (fp64 arithmetic on fp32 inputs is exact here: |x| + 0.5 needs < 53 bits)."""
    x64 = x.astype(np.float64)
    r = np.where(np.abs(x64) < 2.0 ** 23, np.copysign(np.floor(np.abs(x64) + 0.5), x64), x64)
    return r.astype(np.float32)


def fast_round(x):
    return np.trunc(x + np.copysign(HALF_PRED, x))          # fp32 + fp32 -> fp32, round to nearest even


def check(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        a, b = fast_round(x), c_round(x)
    fin = np.isfinite(x)
    # same value AND same sign of zero is not needed (the conversion to int drops it), same value is
    bad = fin & (a != b)
    assert not bad.any(), (x[bad][:8], a[bad][:8], b[bad][:8])
    # non-finite inputs pass through both forms unchanged
    assert np.array_equal(np.isnan(a[~fin]), np.isnan(x[~fin])) and np.array_equal(np.isnan(b[~fin]), np.isnan(x[~fin]))
    inf = np.isinf(x)
    assert np.array_equal(a[inf], x[inf]) and np.array_equal(b[inf], x[inf])
    return int(x.size)


def test_the_constant_is_the_fp32_value_below_one_half():
    assert HALF_PRED == np.nextafter(np.float32(0.5), np.float32(0)) and HALF_PRED < np.float32(0.5)
    # 0.5 itself would be wrong: the value just below one half must round to 0
    x = np.nextafter(np.float32(0.5), np.float32(0))
    assert np.trunc(x + np.float32(0.5)) == 1.0 and fast_round(np.array([x]))[0] == 0.0


def test_every_half_integer_and_its_neighbours_below_2_23():
    n_checked = 0
    step = 1 << 20
    for lo in range(0, 1 << 23, step):
        n = np.arange(lo, lo + step, dtype=np.float64)
        for h in (n - 0.5, n, n + 0.5):
            h = h.astype(np.float32)                                   # exact: |h| < 2^23 has a representable .5
            for v in (h, np.nextafter(h, np.float32(-np.inf)), np.nextafter(h, np.float32(np.inf))):
                n_checked += check(v) + check(-v)
    assert n_checked == 2 * 9 * (1 << 23)


def test_zeros_subnormals_large_values_inf_nan():
    tiny = np.frombuffer(np.arange(0, 1 << 16, dtype=np.uint32).tobytes(), dtype=np.float32)          # +0 and the smallest subnormals
    top_sub = np.frombuffer(np.arange((1 << 23) - 4096, (1 << 23) + 4096, dtype=np.uint32).tobytes(), dtype=np.float32)   # subnormal / normal border
    check(tiny), check(-tiny), check(top_sub), check(-top_sub)
    for e in range(-3, 33):
        p = np.float32(2.0 ** e)
        bits = int(np.array([p]).view(np.uint32)[0])
        nb = np.arange(bits - 4096, bits + 4096, dtype=np.uint32).view(np.float32)               # 4096 values on either side of 2^e
        check(nb), check(-nb)
    check(np.array([np.inf, -np.inf, np.nan, -np.nan, np.finfo(np.float32).max, -np.finfo(np.float32).max, 0.0, -0.0], dtype=np.float32))
    rng = np.random.default_rng(5)
    check(rng.integers(0, 1 << 32, size=1 << 22, dtype=np.uint64).astype(np.uint32).view(np.float32))      # and a random sample of all patterns


def exhaustive(chunk=1 << 24):
    n = 0
    for lo in range(0, 1 << 32, chunk):
        n += check(np.arange(lo, lo + chunk, dtype=np.uint64).astype(np.uint32).view(np.float32))
    return n


if __name__ == '__main__':
    if '--exhaustive' in sys.argv:
        import time
        t0 = time.time()
        print(f'all fp32 bit patterns: {exhaustive()} checked, 0 mismatches, {time.time() - t0:.0f} s')
