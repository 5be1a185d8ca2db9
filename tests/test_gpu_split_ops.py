"""VITS_ARITH_F32_SPLIT at operator level (vits.cpp_amd/csrc/conv_split.hip through vits_op_conv1d / vits_op_resblock_pair, which run the engine's own launch
sequence or refuse): one conv and one ResBlock pair against a numpy float64 reference of the same fp32 inputs, at the resolution where "fp32-accurate" can be false.

Bound — derived per case, not a fixed number (tests/split_ref.py): the rms error of the GPU result <= 2 x the rms error of a sequential fp32 fmaf chain computed in
numpy on the same data, both against the float64 result and relative to its RMS. A kernel that loses one of the small cross products (a2 w2, a3 w1) sits at 3-8 x
the chain, the correct arithmetic in its worst summation order at 1.7 x (tests/test_split_emulation.py asserts both); the whole-model bounds of
tests/test_gpu_split.py (1e-4, 5e-5 of RMS) are five to ten times too wide to see such a loss. The chain runs on a fixed, evenly spread subset of output channels
with at least 8192 outputs — on every output where a case has fewer (the short-T cases: 384 to 2048 outputs; the sampling noise of an RMS over N values is
1 / sqrt(2 N) <= 4 %, far inside the factor). Where a 32-row tile of the grid has 8192 outputs of its own it is held to the same rule by itself, so that a fault in
one row block is not diluted by the others.

The op fills the three-plane input buffers with bf16 NaNs before the converter runs, so a read of a slot past an utterance's length is a NaN in the result; columns
past lens[b] must come back untouched (zero). Every case prints its max error and its ratio to the chain."""
import numpy as np
import pytest

import split_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu
SLOPE = 0.1


@pytest.fixture(autouse=True)
def _split_op_arith(pkg):
    pkg.op_set_arith(pkg.ARITH_F32_SPLIT)
    yield
    pkg.op_set_arith(pkg.ARITH_F32)


hold_to_the_chain = R.hold_to_the_chain


def check_conv(pkg, cin, cout, k, dil, T, lens, pre_slope=None, residual=False, accum=False, out_scale=1.0, bf16_weights=False, edit_w=None, label=""):
    x, w, bias, res, acc = R.make_case(cin, cout, k, dil, T, len(lens), bf16_weights=bf16_weights)
    if edit_w:
        edit_w(w)
    got = pkg.op_conv1d(x, w, bias, dilation=dil, pre_slope=pre_slope, residual=res if residual else None, accum=acc if accum else None, out_scale=out_scale,
                        lens=lens)
    A = R.im2col(x if pre_slope is None else R.lrelu32(x, pre_slope), lens, k, dil)
    rc = R.gather_cols(res, lens) if residual else None
    ac = R.gather_cols(acc, lens) if accum else None
    ref = R.epilogue64(R.conv64(w, A), bias, rc, ac, out_scale)
    rows = R.chain_rows(cout, A.shape[1])
    chain = R.epilogue32(R.chain32(w.reshape(cout, -1)[rows], A), bias[rows], None if rc is None else rc[rows], None if ac is None else ac[rows], out_scale)
    return hold_to_the_chain("conv %dx%d k%d d%d T%d %s" % (cin, cout, k, dil, T, label), got, lens, ref, chain, rows)


@pytest.mark.parametrize("k", [3, 7, 11])
@pytest.mark.parametrize("dil", [1, 3, 5])
def test_every_tap_count_and_dilation_at_128_channels(pkg, k, dil):
    """all nine instantiations; n = 384 products at k = 3 is where a lost cross term stands out most"""
    check_conv(pkg, 128, 128, k, dil, 300, [300, 263], pre_slope=SLOPE)


@pytest.mark.parametrize("cin,cout,k,dil", [
    (160, 128, 3, 1), (160, 128, 7, 3),  # five chunks: the odd tail of the chunk-pair loop
    (224, 256, 3, 5),                    # seven chunks
    (128, 384, 11, 1),                   # three row blocks (grid.y = 3)
    (256, 256, 11, 5),                   # the widest halo, the longest product sum
])
def test_chunk_counts_and_grids_the_model_never_produces(pkg, cin, cout, k, dil):
    check_conv(pkg, cin, cout, k, dil, 300, [300, 263], pre_slope=SLOPE)


@pytest.mark.parametrize("k,dil", [(11, 5), (3, 1)])
@pytest.mark.parametrize("T", [1, 2, 7, 8, 9, 127, 128, 129, 257])
def test_tile_and_length_edges(pkg, k, dil, T):
    """rows shorter than the 25-sample halo, lengths around the 128-column tile, tiles that start past an utterance's end (lens[2] = 1)"""
    check_conv(pkg, 128, 128, k, dil, T, [T, max(1, T - 3), 1], pre_slope=SLOPE)


@pytest.mark.parametrize("name,kw", [
    ("plain", dict()),
    ("pre_slope+residual", dict(pre_slope=SLOPE, residual=True)),
    ("residual+accum/3", dict(residual=True, accum=True, out_scale=1.0 / 3)),
])
def test_epilogues(pkg, name, kw):
    check_conv(pkg, 128, 128, 7, 3, 333, [333, 100, 1], label=name, **kw)


def test_bf16_valued_weights_have_an_all_zero_second_plane_and_the_same_bound(pkg):
    check_conv(pkg, 128, 128, 7, 3, 300, [300, 263], pre_slope=SLOPE, bf16_weights=True, label="bf16 weights")


def _three_pieces(w):
    w[5, 7, 1] = np.float32(1 + 2.0 ** -9 + 2.0 ** -20)


@pytest.mark.parametrize("cin,cout,k,dil,kw,cause", [
    (96, 128, 3, 1, dict(), "c_in = 96"),
    (128, 192, 3, 1, dict(), "c_out = 192"),
    (128, 128, 5, 1, dict(), "k = 5"),
    (128, 128, 3, 2, dict(), "dilation 2"),
    (128, 128, 3, 1, dict(post_act=1), "post_act"),
    (128, 128, 3, 1, dict(edit=_three_pieces), "not the exact sum of two bf16 values"),
])
def test_refusals_name_their_cause_and_never_fall_back(pkg, cin, cout, k, dil, kw, cause):
    x, w, bias, _, _ = R.make_case(cin, cout, k, dil, 40, 2)
    kw = dict(kw)
    if "edit" in kw:
        kw.pop("edit")(w)
    with pytest.raises(pkg.VitsError) as e:
        pkg.op_conv1d(x, w, bias, dilation=dil, lens=[40, 33], **kw)
    assert "VITS_ARITH_F32_SPLIT" in str(e.value) and cause in str(e.value), str(e.value)


def test_a_weight_of_1_plus_2_to_the_minus_20_is_two_bf16_values_and_is_computed_exactly(pkg):
    """1 + 2^-20 has 21 significant bits, but the pieces carry their own exponents: it is bf16(1) + bf16(2^-20), pack_conv_weights_split takes it, and the kernel
    must then get it right (the rule of refusal is `not two bf16 pieces`, which this value does not meet; 1 + 2^-9 + 2^-20 in the refusals above does)."""
    def edit(w):
        w[5, 7, 1] = np.float32(1 + 2.0 ** -20)
    check_conv(pkg, 128, 128, 3, 1, 300, [300, 263], pre_slope=SLOPE, edit_w=edit, label="w = 1 + 2^-20")


# ---- the conv pair of a ResBlock: the epilogue that writes the next conv's planes, and the conv that reads planes an epilogue wrote --------------------------
make_pair = R.make_pair


def check_pair(pkg, C, k, dil, T, label=""):
    lens = [T, max(1, 2 * T // 3), max(1, T // 4)]
    x, w1, b1, w2, b2 = make_pair(C, k, dil, T, len(lens))
    got = pkg.op_resblock_pair(x, w1, b1, w2, b2, dil, SLOPE, lens=lens)
    ref, chain, rows = R.pair_reference(x, w1, b1, w2, b2, lens, dil, SLOPE)
    return hold_to_the_chain("pair C%d k%d d%d T%d %s" % (C, k, dil, T, label), got, lens, ref, chain, rows)


@pytest.mark.parametrize("C", [128, 256])
@pytest.mark.parametrize("k,dil", [(3, 1), (7, 3), (11, 5)])
@pytest.mark.parametrize("T", [9, 130, 300])
def test_resblock_pair_through_the_plane_writing_epilogue(pkg, C, k, dil, T):
    check_pair(pkg, C, k, dil, T)


def test_resblock_pair_in_exact_fp32_and_its_refusal_in_the_16_bit_modes(pkg):
    """the same entry point on the fp32 MFMA kernels (an fmaf chain in a blocked order: the same rule), and a different result from the split run"""
    lens = [130, 86, 32]
    x, w1, b1, w2, b2 = make_pair(128, 7, 3, 130, 3)
    split = pkg.op_resblock_pair(x, w1, b1, w2, b2, 3, SLOPE, lens=lens)
    pkg.op_set_arith(pkg.ARITH_F32)
    check_pair(pkg, 128, 7, 3, 130, label="fp32")
    exact = pkg.op_resblock_pair(x, w1, b1, w2, b2, 3, SLOPE, lens=lens)
    assert not np.array_equal(split, exact)  # two summation orders: the split run was not the fp32 kernels
    for arith in (pkg.ARITH_F16, pkg.ARITH_BF16):
        pkg.op_set_arith(arith)
        with pytest.raises(pkg.VitsError, match="VITS_ARITH_F32 or VITS_ARITH_F32_SPLIT only"):
            pkg.op_resblock_pair(x, w1, b1, w2, b2, 3, SLOPE, lens=lens)
    pkg.op_set_arith(pkg.ARITH_F32_SPLIT)
    with pytest.raises(pkg.VitsError, match="c_in = 64"):
        pkg.op_resblock_pair(x[:, :64], w1[:64, :64], b1[:64], w2[:64, :64], b2[:64], 3, SLOPE, lens=lens)
    with pytest.raises(pkg.VitsError, match="VITS_ARITH_F32_SPLIT: the transposed conv has no split kernel"):
        pkg.op_conv_transpose1d(x, np.zeros((128, 8, 4), np.float32), None, 2, 1)


# ---- whole model, bf16-stored weights (second weight plane all zero) -----------------------------------------------------------------------------------------
def test_split_arithmetic_on_a_model_with_bf16_stored_weights(pkg, oracle):
    data = pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL | pkg.SYNTH_BF16)
    om = oracle.Model(data)
    Ts = [12, 7, 9]
    ids = np.zeros((3, 12), np.int32)
    for b, T in enumerate(Ts):
        ids[b, :T] = pkg.synth_ids(1, T, ids_seed=520 + b)[0]
    with pkg.Model(data) as m:
        exact, le, fe = m.process_batch(ids, id_lengths=Ts, noise_seed=23)
        m.set_arith(pkg.ARITH_F32_SPLIT)
        assert m.arith == pkg.ARITH_F32_SPLIT
        pcm, lengths, frames = m.process_batch(ids, id_lengths=Ts, noise_seed=23, collect_taps=True)
        assert np.array_equal(lengths, le) and np.array_equal(frames, fe)
        worst = 0.0
        for b, T in enumerate(Ts):
            ref = om.process_ids(ids[b, :T], noise_kind=oracle.NOISE_COUNTER, noise_seed=23 + b)
            assert np.array_equal(m.tap("durations", b), ref["durations"])
            assert pcm[b].size == ref["waveform"].size == lengths[b]
            for name in ("z_flow", "pre_tanh", "waveform"):
                e = rel_err(m.tap(name, b), ref[name])
                worst = max(worst, e)
                assert e < 1e-4, (b, name, e)
            assert not np.array_equal(pcm[b], exact[b])  # the split kernels ran on the bf16-stored weights: another summation order than the exact path
        print("split arithmetic, bf16-stored weights: max tap error vs the fp32 oracle %.2e of RMS" % worst)
