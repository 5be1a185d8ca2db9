"""The HiFiGAN upsamplers of the 16-bit modes at operator level (convt16.hip: convt16_kernel<NR, CSPLIT, RS, BF>, convt16_lines_kernel<64 | 128, BF>, and the GEMM-tile
form they claim to be bit-identical to, conv16_kernel<2, -1, ..., E16_CONVT_GROUP>, through vits_op_upsample16), at lengths no whole model produces. A model gives
these kernels its four layer shapes at the lengths the duration predictor happens to choose; here every instantiation runs at the smallest shape that reaches it
(CASES), and at every length where its code takes another path: the one-position last tile, the 32- and 64-column and column-split boundaries, partly valid quads of
the lines kernels' transpose, one position short of / exactly / one past a block, and a third block (lengths_of). The batch is ragged, lens = [t, max(t - 1, 1),
(t + 1) // 2, 0]; the op stages 0xFF bytes behind lens[b] in the 16-bit input and zeros in the outputs.

Each test asserts the kernel name of the plan BEFORE it runs a case, so that no case can pass on another kernel. What is asserted, per variant (1 = GEMM tile,
2 = streaming) and per forced split of the lines kernels' deal over gridDim.z:
  1. no NaN in a valid output (nothing was read past lens[b]);
  2. every element of y and y16 at n >= len_out[b] is still zero, the whole row of the utterance with lens = 0 included;
  3. anchor: max error < 2e-5 of RMS per utterance against the float64 reference on the same rounded operands (tests/upsample_ref.py) — the project's bound for
     these MFMA instructions (tests/test_gpu_arith16.py, tests/test_gpu_ops.py); the ratio of the GPU's rms error to that of the sequential fp32 chain is printed,
     not asserted;
  4. the 16-bit copy is exactly the type's rounding of leaky_relu(y_gpu, y16_slope) of the fp32 value stored beside it, at slopes 0.1 and 1.0;
  5. the converter's output is exactly the rounding of leaky_relu(x, pre_slope) on t < lens[b] and still 0xFFFF behind it;
  6. bit identity: variant 2 == variant 1, every forced split == split 1, variant 0 == the variant its plan names.
tests/test_upsample_op_host.py checks this file's case table, the plans and the refusals on the CPU."""
import numpy as np
import pytest

import split_ref as R
import upsample_ref as U
from conftest import rel_err

pytestmark = pytest.mark.gpu
F32, BF16, F16, SPLIT = 0, 1, 2, 3  # pkg.ARITH_*
ARITH_NAME = {F16: "f16", BF16: "bf16"}
PLAN, TILE, STREAM = 0, 1, 2  # pkg.UP16_VARIANT_*
PRE_SLOPE = 0.1
BOUND = 2e-5


def _case(cin, cout, stride, stream, splits=()):
    return dict(cin=cin, cout=cout, stride=stride, stream=stream, splits=tuple(splits))


# (c_in, c_out, stride): the smallest shape that reaches each instantiation; `stream` = the streaming kernel's name without the operand type; `splits` = forced deals
CASES = [
    _case(64, 32, 2, "convt16_kernel<4, 2, 8, "),      # 256 positions per block, two waves per row tile
    _case(128, 32, 2, "convt16_kernel<4, 2, 16, "),    # the 16-slot ring
    _case(64, 32, 1, "convt16_kernel<4, 2, 8, "),      # one row tile: waves 2 and 3 have no pass
    _case(64, 64, 2, "convt16_kernel<4, 1, 8, "),      # 128 positions per block
    _case(64, 32, 3, "convt16_kernel<4, 1, 8, "),      # three row tiles (wave 3 idle), phase = row / c_out with an odd stride, odd crop
    _case(128, 64, 2, "convt16_kernel<4, 1, 16, "),    # the model's third upsampler
    _case(320, 64, 2, "convt16_kernel<2, 1, 8, "),     # 64 positions per block, 40 k-steps
    _case(512, 64, 2, "convt16_kernel<2, 1, 16, "),    # LDS above 64 KB
    _case(64, 64, 4, "convt16_lines_kernel<128, "),    # 4 units, gridDim.z 1
    _case(128, 64, 8, "convt16_lines_kernel<128, ", splits=(1, 4)),   # 8 units: the planner's gridDim.z 2
    _case(256, 128, 8, "convt16_lines_kernel<128, ", splits=(1, 2)),  # the model's second upsampler, 16 units: the planner's gridDim.z 4
    _case(320, 32, 8, "convt16_lines_kernel<64, ", splits=(1, 2)),    # 2 units for 4 waves; split 2: a block without a unit
    _case(512, 256, 8, "convt16_lines_kernel<64, ", splits=(1, 4)),   # the model's first upsampler
    _case(64, 32, 5, None),                             # 160 rows, stride % 4 != 0: no streaming kernel, variant 0 is the GEMM tile
]
PLANNER_GZ = {(64, 64, 4): 1, (128, 64, 8): 2, (256, 128, 8): 4, (320, 32, 8): 1, (512, 256, 8): 4}  # gridDim.z of the lines kernels on a small grid
ARITHS = (F16, BF16)


def case_id(c):
    return "c%dx%d-s%d" % (c["cin"], c["cout"], c["stride"])


def crops_of(c):
    s = c["stride"]
    return sorted({0, (2 * s - s) // 2})


def expected_stream_kernel(c, arith):
    return None if c["stream"] is None else c["stream"] + ("true>" if arith == BF16 else "false>")


def plan_of(pkg, c, arith, t=1, batch=4, variant=PLAN, split=0, crop=0):
    pkg.op_set_arith(arith)
    try:
        return pkg.op_upsample16_plan(c["cin"], c["cout"], c["stride"], t, batch=batch, crop=crop, variant=variant, split=split)
    finally:
        pkg.op_set_arith(F32)


def lengths_of(bn):
    return sorted({1, 2, 3, 5, 6, 31, 32, 33, 63, 64, 65, bn - 1, bn, bn + 1, 2 * bn + 3})


def ragged(t):
    return [t, max(t - 1, 1), (t + 1) // 2, 0]


def valid_out(L, stride, crop):
    """output samples of an utterance of L positions: an empty utterance gets no store at all"""
    return U.out_len(L, stride, crop) if L > 0 else 0


# ---- data and references, one per (shape, t) / (arithmetic, shape, t), shared by the variants, splits and crops of a case ------------------------------------------
_DATA, _REF = {}, {}


def data_of(c, t):
    key = (c["cin"], c["cout"], c["stride"], t)
    if key not in _DATA:
        rng = np.random.default_rng(R.case_seed(c["cin"], c["cout"], 2 * c["stride"], c["stride"], t) + 11)
        x = rng.standard_normal((4, c["cin"], t)).astype(np.float32)
        w = (rng.standard_normal((c["cin"], c["cout"], 2 * c["stride"])) / np.sqrt(2 * c["cin"])).astype(np.float32)
        bias = rng.standard_normal(c["cout"]).astype(np.float32)
        _DATA[key] = (x, w, bias)
    return _DATA[key]


def reference_of(c, arith, t, lens, with_bias=True):
    """per utterance: (float64 un-cropped [c_out, s (L + 1)], chain fp32 on `channels`, channels) — None for an empty utterance"""
    key = (arith, c["cin"], c["cout"], c["stride"], t, tuple(lens), with_bias)
    if key not in _REF:
        x, w, bias = data_of(c, t)
        xr, wr = U.operands(x, w, PRE_SLOPE, arith)
        out = []
        for b, L in enumerate(lens):
            if L == 0:
                out.append(None)
                continue
            ch = U.chain_channels(c["cout"], c["stride"] * (L + 1))
            bb = bias if with_bias else None
            out.append((U.upsample64(xr[b, :, :L], wr, bb, c["stride"]), U.upsample_chain32(xr[b, :, :L], wr, bb, c["stride"], ch), ch))
        _REF[key] = out
    return _REF[key]


def run(pkg, c, arith, t, lens, crop, variant, split=0, y16_slope=0.1, **kw):
    x, w, bias = data_of(c, t)
    pkg.op_set_arith(arith)
    return pkg.op_upsample16(x[: len(lens)], w, bias, c["stride"], crop, pre_slope=PRE_SLOPE, y16_slope=y16_slope, variant=variant, split=split, lens=lens, **kw)


class Errors:
    """squared errors of a case pooled over its lengths: the GPU's on every output, the chain's on its channels, each relative to the reference's RMS there"""

    def __init__(self):
        self.g = self.rg = self.c = self.rc = 0.0
        self.worst = 0.0

    def add(self, got, ref, chain, channels):
        eg, rg = float(((got.astype(np.float64) - ref) ** 2).sum()), float((ref ** 2).sum())
        ec, rc = float(((chain.astype(np.float64) - ref[channels]) ** 2).sum()), float((ref[channels] ** 2).sum())
        self.g, self.rg, self.c, self.rc = self.g + eg, self.rg + rg, self.c + ec, self.rc + rc
        if ec > 0 and got.size >= 4096:
            self.worst = max(self.worst, np.sqrt(eg / rg) / np.sqrt(ec / rc))

    def ratio(self):
        return np.sqrt(self.g / self.rg) / (np.sqrt(self.c / self.rc) + 1e-300)


def check(label, res, refs, lens, c, arith, crop, y16_slope, errors=None):
    """assertions 1-4 on one result"""
    y, y16 = res["y"], res.get("y16")
    for b, L in enumerate(lens):
        lo = valid_out(L, c["stride"], crop)
        assert not y[b, :, lo:].any(), (label, b, "y was written at n >= len_out[b]")
        assert y16 is None or not y16[b, :, lo:].any(), (label, b, "y16 was written at n >= len_out[b]")
        if lo == 0:
            continue
        got = y[b, :, :lo]
        assert np.isfinite(got).all(), (label, b, "a slot past lens[b] (NaN) was read", np.argwhere(~np.isfinite(got))[:4].tolist())
        ref64, chain, channels = refs[b]
        ref = U.crop_cols(ref64, crop)
        err = rel_err(got, ref)
        assert err < BOUND, (label, "utterance", b, "len", L, err)
        if errors is not None:
            errors.add(got, ref, U.crop_cols(chain, crop), channels)
        if y16 is not None:
            want = U.y16_bits(got, y16_slope, arith)
            if not np.array_equal(y16[b, :, :lo], want):
                bad = np.argwhere(y16[b, :, :lo] != want)
                raise AssertionError((label, b, "y16 is not the rounding of leaky_relu(y, %g): %d values, first at %s" % (y16_slope, len(bad), bad[0].tolist())))


def same_bits(label, got, want):
    for name in ("y", "y16"):
        if name in got and name in want and not np.array_equal(got[name], want[name]):
            bad = np.argwhere(got[name] != want[name])
            raise AssertionError((label, name, "%d values differ; rows %d..%d, channels %d..%d, samples %d..%d" % (
                len(bad), bad[:, 0].min(), bad[:, 0].max(), bad[:, 1].min(), bad[:, 1].max(), bad[:, 2].min(), bad[:, 2].max())))


@pytest.fixture(autouse=True)
def _reset_op_arith(pkg):
    yield
    pkg.op_set_arith(pkg.ARITH_F32)


def assert_plans(pkg, c, arith):
    """the kernel every variant of the case runs, asserted before anything is launched; returns (streaming?, bn)"""
    want = expected_stream_kernel(c, arith)
    p1 = plan_of(pkg, c, arith, variant=TILE)
    assert p1["variant"] == TILE and p1["kernel"].startswith("conv16_kernel<2, -1, ") and p1["kernel"].endswith(", 4, %s>" % ("true" if arith == BF16 else "false")), p1
    p0 = plan_of(pkg, c, arith, variant=PLAN)
    if want is None:
        assert p0["variant"] == TILE and p0["kernel"] == p1["kernel"], p0
        with pytest.raises(pkg.VitsError) as e:
            plan_of(pkg, c, arith, variant=STREAM)
        assert "stride is not a multiple of 4" in str(e.value), str(e.value)
        return False, p1["bn"]
    p2 = plan_of(pkg, c, arith, variant=STREAM)
    assert p2["variant"] == STREAM and p2["kernel"] == want, (p2, want)
    assert p0["variant"] == STREAM and p0["kernel"] == want and p0["grid"] == p2["grid"], p0
    key = (c["cin"], c["cout"], c["stride"])
    assert p2["grid"][2] == PLANNER_GZ.get(key, 1), p2
    for split in c["splits"]:
        ps = plan_of(pkg, c, arith, variant=STREAM, split=split)
        assert ps["kernel"] == want and ps["grid"] == (p2["grid"][0], p2["grid"][1], split), ps
    return True, p2["bn"]


@pytest.mark.parametrize("arith", ARITHS, ids=lambda a: ARITH_NAME[a])
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_upsampler_at_every_length_edge(pkg, c, arith):
    stream, bn = assert_plans(pkg, c, arith)
    named = STREAM if stream else TILE
    label0 = "%s-%s" % (case_id(c), ARITH_NAME[arith])
    errors = Errors()
    for t in lengths_of(bn):
        lens = ragged(t)
        refs = reference_of(c, arith, t, lens)
        for crop in crops_of(c):
            label = "%s t %d crop %d" % (label0, t, crop)
            tile = run(pkg, c, arith, t, lens, crop, TILE)
            check(label + " variant 1", tile, refs, lens, c, arith, crop, 0.1, errors)
            if stream:
                got = run(pkg, c, arith, t, lens, crop, STREAM)
                check(label + " variant 2", got, refs, lens, c, arith, crop, 0.1)
                same_bits(label + " variant 2 vs variant 1", got, tile)
                base = None
                for split in c["splits"]:
                    part = run(pkg, c, arith, t, lens, crop, STREAM, split=split)
                    check(label + " split %d" % split, part, refs, lens, c, arith, crop, 0.1)
                    base = part if base is None else base
                    same_bits(label + " split %d vs split %d" % (split, c["splits"][0]), part, base)
                    same_bits(label + " split %d vs the planner's" % split, part, got)
            # the 16-bit copy without its leaky ReLU: the same fp32 bits beside it
            plain = run(pkg, c, arith, t, lens, crop, named, y16_slope=1.0)
            check(label + " y16_slope 1", plain, refs, lens, c, arith, crop, 1.0)
            assert np.array_equal(plain["y"], tile["y"]), (label, "y16_slope changed y")
            if t in (1, bn + 1, 2 * bn + 3):
                same_bits(label + " variant 0 vs the variant its plan names", run(pkg, c, arith, t, lens, crop, PLAN), got if stream else tile)
    print("%s: gpu rms error / sequential fp32 chain rms error: %.3f pooled over the lengths, worst single length %.3f (gpu rms %.2e of RMS)" % (
        label0, errors.ratio(), errors.worst, np.sqrt(errors.g / errors.rg)))


@pytest.mark.parametrize("arith", ARITHS, ids=lambda a: ARITH_NAME[a])
def test_converter_output_is_the_exact_rounding_and_nothing_behind_lens(pkg, arith):
    c = CASES[0]
    assert_plans(pkg, c, arith)
    t = 33
    lens = ragged(t)
    x, _, _ = data_of(c, t)
    res = run(pkg, c, arith, t, lens, 0, STREAM, want_x16=True)
    want = U.bits16(R.lrelu32(x, PRE_SLOPE), arith)
    for b, L in enumerate(lens):
        assert np.array_equal(res["x16"][b, :, :L], want[b, :, :L]), (b, "the converter's output is not round16(leaky_relu(x))")
        assert (res["x16"][b, :, L:] == 0xFFFF).all(), (b, "the converter wrote behind lens[b]")


@pytest.mark.parametrize("arith", ARITHS, ids=lambda a: ARITH_NAME[a])
@pytest.mark.parametrize("c", [CASES[5], CASES[8]], ids=case_id)  # one per kernel family: convt16_kernel<4, 1, 16>, convt16_lines_kernel<128>
def test_strides_no_bias_and_a_batch_of_one(pkg, c, arith):
    """rows longer than t / t_out with garbage behind them, bias = None, a batch of 1 without lens, and the call without a 16-bit destination"""
    _, bn = assert_plans(pkg, c, arith)
    t, s = bn + 5, c["stride"]
    crop = crops_of(c)[-1]
    lens = ragged(t)
    x, w, bias = data_of(c, t)
    t_out = U.out_len(t, s, crop)
    pkg.op_set_arith(arith)
    plain = {v: run(pkg, c, arith, t, lens, crop, v) for v in (TILE, STREAM)}
    xw = np.concatenate([x, np.full((4, c["cin"], 5), 7.5, np.float32)], axis=2)
    for v in (TILE, STREAM):
        wide = pkg.op_upsample16(xw, w, bias, s, crop, variant=v, lens=lens, t=t, t_out_stride=t_out + 7)
        assert np.array_equal(wide["y"][:, :, :t_out], plain[v]["y"]) and np.array_equal(wide["y16"][:, :, :t_out], plain[v]["y16"]), ("strides changed the result", v)
        assert not wide["y"][:, :, t_out:].any() and not wide["y16"][:, :, t_out:].any()
        no16 = run(pkg, c, arith, t, lens, crop, v, want_y16=False)
        assert "y16" not in no16 and np.array_equal(no16["y"], plain[v]["y"]), ("the call without a 16-bit destination changed y", v)
    refs = reference_of(c, arith, t, lens, with_bias=False)
    res = {v: pkg.op_upsample16(x, w, None, s, crop, variant=v, lens=lens) for v in (TILE, STREAM)}
    for v in (TILE, STREAM):
        check("bias = None, variant %d" % v, res[v], refs, lens, c, arith, crop, 0.1)
    same_bits("bias = None", res[STREAM], res[TILE])
    refs1 = reference_of(c, arith, t, [t])
    one = {v: pkg.op_upsample16(x[:1], w, bias, s, crop, variant=v) for v in (TILE, STREAM)}
    for v in (TILE, STREAM):
        check("batch 1 without lens, variant %d" % v, one[v], refs1, [t], c, arith, crop, 0.1)
        assert np.array_equal(one[v]["y"][0], plain[v]["y"][0]) and np.array_equal(one[v]["y16"][0], plain[v]["y16"][0]), ("a row of the ragged batch != its batch-1 call", v)
    same_bits("batch 1 without lens", one[STREAM], one[TILE])


REFUSALS = [
    # (arith, c_in, c_out, stride, variant, split, what the message names)
    (F32, 64, 32, 2, PLAN, 0, "vits_op_conv_transpose1d"),
    (SPLIT, 128, 128, 2, TILE, 0, "vits_op_conv_transpose1d"),
    (F16, 96, 32, 2, STREAM, 0, "c_in is not a multiple of 64"),
    (BF16, 64, 48, 2, STREAM, 0, "c_out is not a multiple of 32"),
    (F16, 576, 32, 2, STREAM, 0, "c_in > 512"),
    (F16, 64, 32, 5, STREAM, 0, "rows = stride x c_out = 160 > 128 and stride is not a multiple of 4"),
    (BF16, 64, 32, 6, STREAM, 0, "stride is not a multiple of 4"),
    (F16, 64, 32, 2, STREAM, 2, "only convt16_lines_kernel"),
    (F16, 64, 64, 4, TILE, 1, "only convt16_lines_kernel"),
    (BF16, 64, 32, 5, PLAN, 2, "only convt16_lines_kernel"),
    (F16, 64, 64, 4, STREAM, 3, "split = 3"),
    (F16, 64, 64, 4, STREAM, 8, "split = 8"),
    (F16, 64, 64, 4, 3, 0, "variant 3"),
    (F16, 64, 36, 2, TILE, 0, "multiples of 8"),
]


def refusal_id(r):
    return "%s-c%dx%d-s%d-v%d-z%d" % ({F32: "f32", SPLIT: "split"}.get(r[0], ARITH_NAME.get(r[0])), r[1], r[2], r[3], r[4], r[5])


def check_refusal(pkg, r):
    """the plan query and the op refuse with the same message, before any device call: this runs without a GPU"""
    arith, cin, cout, s, variant, split, cause = r
    pkg.op_set_arith(arith)
    try:
        with pytest.raises(pkg.VitsError) as e:
            pkg.op_upsample16_plan(cin, cout, s, 40, batch=2, variant=variant, split=split)
        assert "vits_op_upsample16" in str(e.value) and cause in str(e.value), str(e.value)
        x = np.zeros((2, cin, 40), np.float32)
        w = np.zeros((cin, cout, 2 * s), np.float32)
        with pytest.raises(pkg.VitsError) as e2:
            pkg.op_upsample16(x, w, None, s, 0, variant=variant, split=split, lens=[40, 33])
        assert str(e2.value) == str(e.value)
    finally:
        pkg.op_set_arith(F32)


def check_argument_refusals(pkg):
    """lens[b] outside [0, t], and a kernel size the descriptor cannot express: refused before any device call"""
    pkg.op_set_arith(F16)
    try:
        x = np.zeros((2, 64, 40), np.float32)
        w = np.zeros((64, 32, 4), np.float32)
        for lens in ([41, 3], [40, -1]):
            for variant in (PLAN, TILE, STREAM):
                with pytest.raises(pkg.VitsError) as e:
                    pkg.op_upsample16(x, w, None, 2, 0, variant=variant, lens=lens)
                assert "vits_op_upsample16" in str(e.value) and "0 <= lens[b] <= t" in str(e.value), str(e.value)
        for k in (3, 5, 8):  # stride 2: k = 4 only
            with pytest.raises(pkg.VitsError) as e:
                pkg.op_upsample16(x, np.zeros((64, 32, k), np.float32), None, 2, 0, variant=TILE)
            assert "vits_op_upsample16" in str(e.value) and "k = 2 x stride only" in str(e.value), str(e.value)
        with pytest.raises(pkg.VitsError) as e:
            pkg.op_upsample16(x, w, None, 2, 2, variant=TILE)  # crop beyond (k - stride) / 2
        assert "crop = 2" in str(e.value), str(e.value)
    finally:
        pkg.op_set_arith(F32)


@pytest.mark.parametrize("r", REFUSALS, ids=refusal_id)
def test_refusals_name_their_cause_and_never_fall_back(pkg, r):
    check_refusal(pkg, r)


def test_bad_lens_and_kernel_sizes_are_refused(pkg):
    check_argument_refusals(pkg)
