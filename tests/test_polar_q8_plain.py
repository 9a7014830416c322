"""The int8 arithmetic contract on the CPU (no GPU needed): tests/sclist_q8.py, the restatement
that pins the fixed-point decoder (tests/test_polar_q8.py), against tests/sclist_plain.py where the
two must agree, and the numpy quantiser.

Where no g step can saturate the contract is float arithmetic on small integers: with integer
LLRs and U max|llr| <= 127 every value of the recursion is an integer of magnitude <= 127 (a g step
at most doubles a bound that starts at max|llr| and there are log2 U layers), exact in float32, so
both decoders see the same numbers and must give the same lists, metrics included.
"""
import numpy as np
import pytest

import sclist_plain
import sclist_q8
from bchk_pkg import load
from polar_lib import arikan_spec

# n, K, dynamic constraints, max |llr|: U max|llr| = 112 and 96
SMALL = [(4, 8, 0, 7), (4, 9, 3, 7), (5, 16, 0, 3), (5, 14, 4, 3)]


@pytest.mark.parametrize("L", [1, 4, 8])
@pytest.mark.parametrize("n,K,dyn,amp", SMALL)
def test_q8_restatement_equals_the_float_one_without_saturation(n, K, dyn, amp, L):
    U = 1 << n
    assert U * amp <= 127
    spec = arikan_spec(n, K, dyn=dyn, seed=n + dyn)
    rng = np.random.default_rng(100 * n + 10 * dyn + L)
    rows = rng.integers(-amp, amp + 1, (12, U)).astype(np.int8)
    rows[0] = 0                      # every LLR zero: all candidates tie
    rows[1, ::2] = 0
    rows[2] = amp * np.where(rng.integers(0, 2, U) != 0, 1, -1)  # every magnitude equal
    assert (rows == 0).any() and np.abs(rows).max() == amp
    for q in rows:
        wc, wi, ww, wm = sclist_plain.decode(spec, q.astype(np.float32), L)
        gc, gi, gw, gm = sclist_q8.decode(spec, q, L)
        assert gc == wc
        np.testing.assert_array_equal(gi, wi)
        np.testing.assert_array_equal(gw, ww)
        assert gm.dtype == np.int64
        np.testing.assert_array_equal(gm.astype(np.float32).view(np.uint32), wm.view(np.uint32))


def test_q8_steps_saturate_symmetrically():
    a = np.array([127, -127, 100, -100, 0, 5, -5, 0], np.int32)
    b = np.array([127, -127, -100, 100, 9, 0, -7, 0], np.int32)
    np.testing.assert_array_equal(sclist_q8.f_step(a, b), [127, 127, -100, -100, 0, 0, 5, 0])
    np.testing.assert_array_equal(sclist_q8.g_step(a, b, np.zeros(8)), [127, -127, 0, 0, 9, 5, -12, 0])
    np.testing.assert_array_equal(sclist_q8.g_step(a, b, np.ones(8)), [0, 0, -127, 127, 9, -5, -2, 0])


def test_q8_load_rule():
    # -128 reads as -127; shortened symbols +127, punctured ones 0
    spec = arikan_spec(3, 3, punct=(1,), short=(7,), freeze=(7,))
    y, sent = sclist_q8.load_llrs(spec, np.array([-128, 5, -127, 127, 0, -1], np.int8))
    np.testing.assert_array_equal(y, [-127, 0, 5, -127, 127, 0, -1, 127])
    assert sent == [0, 2, 3, 4, 5, 6]


def test_numpy_quantize():
    q = load().quantize
    x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999997, 62.5, 63.5, 1e9, -1e9, np.inf, -np.inf, np.nan,
                  -0.0, 126.5, 127.5], np.float32)
    got = q(x, 1.0)
    assert got.dtype == np.int8
    np.testing.assert_array_equal(got, [0, 2, 2, 0, -2, -2, 0, 62, 63, 63, -63, 63, -63, 0, 0, 63, 63])
    np.testing.assert_array_equal(q(x, 1.0, qmax=127)[-2:], [126, 127])
    np.testing.assert_array_equal(q(x[9:14], 1.0, qmax=127), [127, -127, 127, -127, 0])
    # the product is formed in float32: 0.1f is 0.1 + 1.5e-9, and 5 times it rounds to 0.5 exactly
    # in f32 (a tie, to 0), where the double product 0.5000000075 would round to 1
    assert float(np.float32(0.1)) * 5.0 > 0.5 and np.float32(0.1) * np.float32(5.0) == np.float32(0.5)
    assert q(np.array([0.1, -0.1], np.float32), 5.0).tolist() == [0, 0]
    assert q(np.array([2.5, 3.5], np.float32), 0.5, qmax=127).tolist() == [1, 2]  # 1.25 -> 1, 1.75 -> 2
    # nothing quantises to -128, so the load rule never changes a quantised row
    assert q(np.array([-1e30], np.float32), 1.0, qmax=127)[0] == -127
    for bad in (0, 128, -1):
        with pytest.raises(ValueError, match="qmax"):
            q(x, 1.0, qmax=bad)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="scale"):
            q(x, bad)


def test_q8_refusals_before_the_device(tmp_path):
    F = load()
    with pytest.raises(ValueError, match="q8"):
        F.PolarListDecoder(arikan_spec(5, 16), 4, state="tiered", llr="q8")
    with pytest.raises(ValueError, match="llr"):
        F.PolarListDecoder(arikan_spec(5, 16), 4, llr="int8")
    # a named layer (needs no kernel file): refused with the layer named, before any device call
    named = "12 6 0 3 0 0\nA G A\n" + "".join(f"1 {i}\n" for i in range(6))
    with pytest.raises(F.BchkError, match=r'layer 1 is "G"'):
        F.PolarListDecoder(named, 4, llr="q8")
    with pytest.raises(F.BchkError, match="LDS"):
        F.PolarListDecoder(arikan_spec(13, 4096), 32, llr="q8")
