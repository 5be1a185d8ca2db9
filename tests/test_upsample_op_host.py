"""vits_op_upsample16 without a GPU: the numpy reference of tests/upsample_ref.py against torch's float64 conv_transpose1d; the plan query
(vits_op_upsample16_plan, host arithmetic only) over the case table of tests/test_gpu_upsample_ops.py — imported, not restated — against launch_plan.h's geometry
rules and the frozen launch-plan table; the lengths of a case against its kernel's block; and the refusals, which come back before any device call."""
import os

import numpy as np
import pytest

import split_ref as R
import test_gpu_upsample_ops as G
import upsample_ref as U
from conftest import GOLDEN


@pytest.mark.parametrize("stride", [1, 2, 3, 4, 8])
def test_the_numpy_reference_is_torchs_conv_transpose1d(stride):
    import torch
    rng = np.random.default_rng(100 + stride)
    cin, cout, k = 12, 10, 2 * stride
    w = rng.standard_normal((cin, cout, k))
    bias = rng.standard_normal(cout)
    for L in (1, 2, 3, 7, 32, 33):
        x = rng.standard_normal((cin, L))
        want = torch.nn.functional.conv_transpose1d(torch.from_numpy(x)[None], torch.from_numpy(w), torch.from_numpy(bias), stride=stride)[0].numpy()
        full = U.upsample64(x, w, bias, stride)
        assert full.shape == want.shape == (cout, stride * (L + 1))
        for crop in sorted({0, (k - stride) // 2}):
            got = U.crop_cols(full, crop)
            assert got.shape[1] == U.out_len(L, stride, crop)
            assert np.abs(got - want[:, crop: want.shape[1] - crop]).max() < 1e-12, (stride, L, crop)
        # the chain is the same sum in fp32: close to the float64 result, and not equal to it
        ch = np.arange(cout)
        chain = U.upsample_chain32(x.astype(np.float32), w.astype(np.float32), bias.astype(np.float32), stride, ch)
        ref32 = U.upsample64(x.astype(np.float32), w.astype(np.float32), bias.astype(np.float32), stride)
        assert chain.dtype == np.float32 and R.rms_err(chain, ref32)[1] < 1e-5


def test_the_16_bit_roundings_are_ties_to_even_and_agree_with_their_bit_patterns():
    v = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -0.3, 1e-3, 65504.0, 2.0 ** -8 + 2.0 ** -17, 0.0], np.float32)
    f = U.round16(v, U.F16)
    assert f[1] == 1.0 and f[2] == np.float32(1.0 + 2.0 ** -9)  # ties to even, both ways
    assert np.array_equal(U.bits16(v, U.F16).view(np.float16).astype(np.float32), f)
    b = U.round16(v, U.BF16)
    assert b[6] == np.float32(2.0 ** -8 + 2.0 ** -16) or b[6] == np.float32(2.0 ** -8)  # a tie at 8 bits of mantissa goes to the even neighbour
    assert np.array_equal((U.bits16(v, U.BF16).astype(np.uint32) << 16).view(np.float32), b)
    x = np.random.default_rng(5).standard_normal(4096).astype(np.float32)
    # half an ulp of 8 / of 11 significant bits (normal numbers)
    assert (np.abs(U.round16(x, U.BF16) - x) <= np.abs(x) * 2.0 ** -8).all() and (np.abs(U.round16(x, U.F16) - x)[np.abs(x) > 1e-4] <= np.abs(x)[np.abs(x) > 1e-4] * 2.0 ** -11).all()
    assert np.array_equal(U.y16_bits(x, 1.0, U.F16), U.bits16(x, U.F16))
    assert np.array_equal(U.y16_bits(x, 0.1, U.BF16), U.bits16(np.maximum(x, x * np.float32(0.1)), U.BF16))


# launch_plan.h, restated: convt16_bn, convt16_xw, convt16_lds
def bn_of(kernel):
    args = [a.strip() for a in kernel[kernel.index("<") + 1: kernel.index(">")].split(",")]
    return int(args[0]) if kernel.startswith("convt16_lines_kernel") else int(args[0]) * int(args[1]) * 32


def lds_of(cin, bn):
    return cin // 8 * ((bn + 1 + 7) // 8 * 8) * 16


def golden_ct_rows():
    """the CT rows of the frozen launch-plan table under the default knobs: (cin, cout, stride, T, B) -> (kernel, (gx, gy, gz), block, lds)"""
    rows, section = {}, None
    with open(os.path.join(GOLDEN, "launch_plan_table.txt")) as f:
        for line in f:
            if line.startswith("## "):
                section = line[3:].strip()
            if not line.startswith("CT ") or " | " not in line or (section is not None and section != "default"):
                continue
            left, right = line.strip().split(" | ")
            key, val = left.split(" : ")
            kernel = val.split(" ", 3)[3]
            g = [int(v) for v in right.split()]
            rows[tuple(int(v) for v in key.split()[1:])] = (kernel, tuple(g[:3]), g[3], g[4])
    return rows


@pytest.mark.parametrize("arith", G.ARITHS, ids=lambda a: G.ARITH_NAME[a])
@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_every_case_names_its_kernel_and_its_geometry_is_launch_plan_hs(pkg, c, arith):
    stream, bn = G.assert_plans(pkg, c, arith)
    Ts = G.lengths_of(bn)
    assert {1, 2, 3, 5, 6, 31, 32, 33, 63, 64, 65, bn - 1, bn, bn + 1, 2 * bn + 3} == set(Ts)
    variant = G.STREAM if stream else G.TILE
    if stream:
        want = G.expected_stream_kernel(c, arith)
        assert bn == bn_of(want)
        for split in (0,) + c["splits"]:
            for t in (1, bn - 1, bn, 2 * bn + 3):
                p = G.plan_of(pkg, c, arith, t=t, variant=variant, split=split)
                assert p["kernel"] == want and p["bn"] == bn and p["block"] == 256 and p["lds"] == lds_of(c["cin"], bn), p
                gz = split if split else G.PLANNER_GZ.get((c["cin"], c["cout"], c["stride"]), 1)
                assert p["grid"] == ((t + 1 + bn - 1) // bn, 4, gz), (t, p)  # q runs over [0, t]: one more column than positions
        if (c["cin"], c["cout"], c["stride"]) == (512, 64, 2):
            assert lds_of(512, bn) > 64 * 1024
        assert G.plan_of(pkg, c, arith)["tag"] == ("SL%d" % bn if "lines" in want else "S" + want[want.index("<") + 1: want.rindex(",")].replace(", ", "."))
    else:
        assert bn == 128 and G.plan_of(pkg, c, arith, variant=G.TILE)["block"] == 320
    # the largest staged tensor of the case stays small
    assert 4 * c["cout"] * (c["stride"] * (max(Ts) + 1)) * 4 <= 6 << 20, (c, max(Ts))


def test_the_plans_of_the_models_own_layers_are_the_frozen_tables_rows(pkg):
    rows = golden_ct_rows()
    seen = 0
    for (cin, cout, s, T, B), (kernel, grid, block, lds) in rows.items():
        c = dict(cin=cin, cout=cout, stride=s)
        if not kernel.startswith("convt16"):
            continue
        try:
            p = G.plan_of(pkg, c, G.F16, t=T, batch=B, variant=G.PLAN)
        except pkg.VitsError:
            continue  # (a row of a shape the streaming kernels refuse)
        if p["variant"] != G.STREAM:
            continue
        seen += 1
        assert (p["kernel"], p["grid"], p["block"], p["lds"]) == (kernel, grid, block, lds), ((cin, cout, s, T, B), p)
    assert seen >= 20, seen


@pytest.mark.parametrize("arith", G.ARITHS, ids=lambda a: G.ARITH_NAME[a])
def test_the_checks_catch_the_defects_they_are_for(arith):
    """a result made from the reference passes G.check; each seeded defect — the last position's second tap lost, a tap read from behind lens[b], a store past
    len_out[b], a store into the empty utterance, a 16-bit copy that is truncated instead of rounded, or taken before the leaky ReLU — fails it"""
    c, t, crop, slope = G.CASES[4], 33, 1, 0.1  # stride 3, odd crop
    s = c["stride"]
    lens = G.ragged(t)
    refs = G.reference_of(c, arith, t, lens)
    x, w, bias = G.data_of(c, t)
    xr, wr = U.operands(x, w, G.PRE_SLOPE, arith)

    def result(y_of=lambda b, L: U.crop_cols(refs[b][0], crop).astype(np.float32)):
        y = np.zeros((4, c["cout"], U.out_len(t, s, crop)), np.float32)
        for b, L in enumerate(lens):
            if L:
                y[b, :, :G.valid_out(L, s, crop)] = y_of(b, L)
        y16 = np.zeros(y.shape, np.uint16)
        for b, L in enumerate(lens):
            lo = G.valid_out(L, s, crop)
            y16[b, :, :lo] = U.y16_bits(y[b, :, :lo], slope, arith)
        return {"y": y, "y16": y16}

    G.check("clean", result(), refs, lens, c, arith, crop, slope, G.Errors())

    def lost_tap(b, L):  # q = L sees only x[L - 1] through the second tap: without it the last s samples are the bias alone
        full = U.upsample64(xr[b, :, :L], wr, bias, s)
        full[:, s * L:] = bias[:, None]
        return U.crop_cols(full, crop).astype(np.float32)

    def over_read(b, L):  # x[L] = NaN instead of zero
        xx = np.concatenate([xr[b, :, :L], np.full((c["cin"], 1), np.nan, np.float32)], axis=1)
        return U.crop_cols(U.upsample64(xx, wr, bias, s)[:, : s * (L + 1)], crop).astype(np.float32)

    def stored_past(r):
        r["y"][1, 5, G.valid_out(lens[1], s, crop)] = 0.25
        return r

    def stored_into_empty(r):
        r["y16"][3, 0, 0] = 1
        return r

    def truncated(r):
        v = R.lrelu32(r["y"], slope)
        if arith == U.F16:
            down = np.where(np.abs(v.astype(np.float16).astype(np.float32)) > np.abs(v), np.nextafter(v.astype(np.float16), np.float16(0)), v.astype(np.float16))
            bits = down.view(np.uint16)
        else:
            bits = (v.view(np.uint32) >> 16).astype(np.uint16)
        r["y16"][0] = bits[0]
        return r

    def before_the_relu(r):
        r["y16"][0] = U.bits16(r["y"][0], arith)
        return r

    for name, bad in (("lost tap", result(lost_tap)), ("over-read", result(over_read)), ("stored past", stored_past(result())), ("empty", stored_into_empty(result())),
                      ("truncated", truncated(result())), ("before the relu", before_the_relu(result()))):
        with pytest.raises(AssertionError):
            G.check(name, bad, refs, lens, c, arith, crop, slope)
            pytest.fail("the check let '%s' through" % name, pytrace=False)


def test_the_ragged_batch_has_an_empty_utterance_and_the_ends_differ():
    assert G.ragged(1) == [1, 1, 1, 0] and G.ragged(6) == [6, 5, 3, 0] and G.ragged(259) == [259, 258, 130, 0]
    assert G.valid_out(0, 8, 0) == 0 and G.valid_out(0, 3, 1) == 0 and G.valid_out(5, 3, 1) == 16 and G.valid_out(5, 8, 4) == 40


@pytest.mark.parametrize("r", G.REFUSALS, ids=G.refusal_id)
def test_refusals_come_back_without_a_gpu(pkg, r):
    G.check_refusal(pkg, r)


def test_bad_lens_and_kernel_sizes_are_refused_without_a_gpu(pkg):
    G.check_argument_refusals(pkg)
