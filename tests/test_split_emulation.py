"""The bound of tests/test_gpu_split_ops.py discriminates (CPU; numpy restatement of vits.cpp_amd/csrc/conv_split.hip's arithmetic in tests/split_ref.py).

The GPU tests hold the split kernels to `rms error <= 2 x the rms error of a sequential fp32 fmaf chain`. That rule is worth something only if (a) the arithmetic the
kernels are meant to compute — bf16 round-to-nearest-even pieces, two per weight and three per activation with zero remainders, five exact cross products, fp32
accumulation — passes it even in its worst (sequential) summation order, and (b) the same arithmetic with ANY one of the droppable products missing fails it. Both
are asserted here on the data of the GPU file's smallest and largest product counts (n = c_in x taps = 384 and 2816, the same seeds). Loosening FACTOR until a lost
term passes turns (b) red."""
import numpy as np
import pytest

import split_ref as R

CASES = [(128, 128, 3, 1), (256, 256, 11, 5)]  # n = 384, 2816
T, LENS, SLOPE = 300, [300, 263], 0.1
DROPS = {"a1 w2": (0, 1), "a2 w1": (1, 0), "a2 w2": (1, 1), "a3 w1": (2, 0)}


def test_bf16_rounding_by_bit_operations_is_round_to_nearest_even():
    f = lambda bits: np.array(bits, np.uint32).view(np.float32)
    x = f([0x3F800000, 0x3F808000, 0x3F818000, 0x3F808001, 0x3F817FFF, 0xBF808000, 0x3F80FFFF])
    want = f([0x3F800000, 0x3F800000, 0x3F820000, 0x3F810000, 0x3F810000, 0xBF800000, 0x3F810000])  # ties go to the even 16-bit pattern
    assert np.array_equal(R.bf16_rne(x), want)
    rng = np.random.default_rng(5)
    v = rng.standard_normal(4096).astype(np.float32)
    (p1, p2, p3), rem = R.split_pieces(v, 3)
    assert not rem.any() and np.array_equal((p1.astype(np.float64) + p2 + p3).astype(np.float32), v)
    h = v.astype(np.float16).astype(np.float32)
    (w1, w2), rem = R.split_pieces(h, 2)
    assert not rem.any() and np.array_equal(w1 + w2, h)
    # every piece has its own exponent: 1 + 2^-20 IS two bf16 values (1 and 2^-20) although it has 21 significant bits; 1 + 2^-9 + 2^-20 needs three
    assert not R.split_pieces(np.float32([1 + 2.0 ** -20]), 2)[1].any()
    assert R.split_pieces(np.float32([1 + 2.0 ** -9 + 2.0 ** -20]), 2)[1].any()


@pytest.mark.parametrize("cin,cout,k,dil", CASES)
def test_five_terms_pass_the_2x_rule_and_every_lost_term_fails_it(cin, cout, k, dil):
    x, w, _, _, _ = R.make_case(cin, cout, k, dil, T, len(LENS))
    A = R.im2col(R.lrelu32(x, SLOPE), LENS, k, dil)
    rows = R.chain_rows(cout, A.shape[1])
    assert rows.size * A.shape[1] >= R.MIN_ELEMS
    W = w.reshape(cout, -1)[rows]
    ref = R.conv64(W, A)
    chain, _ = R.rms_err(R.chain32(W, A), ref)
    names = [None] + list(DROPS)
    results = R.emulate_split(W, A, [None] + list(DROPS.values()))
    full, full_max = R.rms_err(results[0], ref)
    print("n = %d: fp32 chain %.2e of RMS; split, five terms %.2e (max %.2e) = %.2f x the chain" % (cin * k, chain, full, full_max, full / chain))
    assert full <= R.FACTOR * chain, (full, chain)
    for name, got in zip(names[1:], results[1:]):
        e, emax = R.rms_err(got, ref)
        print("    without %s: %.2e (max %.2e) = %.2f x the chain" % (name, e, emax, e / chain))
        assert e > R.FACTOR * chain, (name, e, chain)
