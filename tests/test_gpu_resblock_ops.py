"""The fused ResBlock kernels at operator level (rbpair32_kernel, rbblock32_kernel, rbpair16_kernel, rbblock16_kernel and its segment form, through vits_op_resblock),
at sequence ends and tile edges that no whole model produces: a model feeds every stage a multiple of its upsampling product, so the C = 256 stage never sees a
length that is not a multiple of 8 (the C = 32 stage: of 256), and the tile widths of launch_plan.h meet such lengths only at multiples of 8.

Every case of CASES names one kernel (variant, tiles, nr); vits_op_resblock_plan says which instantiation that is, its tile width `bo`, halo and segment width, and
the lengths are derived from those per case (lengths_of). The batch is lens = [T, T - 1, T - 2, T - 3] (clipped at 1): the sequence end on every residue mod 4.

What is asserted:
  * bit identity, no tolerance: every fused variant == variant 1 (two conv launches per pair, as the engine builds them) on every valid column, and variant 1 == the
    composition of vits_op_conv1d calls (two per pair: pre_slope, residual, accum / out_scale on the last pair) in the same arithmetic — fp32, f16, bf16; the
    scale_div form among the variants only;
  * fp32 anchor: the fused pair (variant 2, one pair) against numpy float64 under the rule of tests/split_ref.py — rms error <= FACTOR x the sequential fp32 chain —
    overall, per 32-row tile, and on the edge windows alone (the last k - 1 columns of every row, k - 1 columns on each side of every tile boundary), pooled per case.
    Whole blocks are bit-identical to pairs that carry the bound;
  * 16-bit anchor: each of the two vits_op_conv1d calls of a pair against the oracle's conv in the same arithmetic on the same operands, 2e-5 of RMS (the bound of
    tests/test_gpu_arith16.py), at these lengths and ragged lens. (No rms-ratio rule for a 16-bit pair: isolated rounding flips of the 16-bit intermediate dominate
    the ratio of two accumulation orders — 0.02 to 1.56 over eight emulated cases.)
  * hygiene: results finite (the op stages NaNs behind every lens[b]), nothing written past lens[b], a row of the ragged batch == its batch-1 call, t_stride > t and
    a t_stride that is no multiple of 4 give the same bits, refusals name their cause, the plan query names the kernel that was asked for.
tests/test_resblock_op_host.py checks this file's own case table and lengths on the CPU."""
import numpy as np
import pytest

import split_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu
SLOPE = 0.1
F32, BF16, F16 = 0, 1, 2  # pkg.ARITH_*
ARITH_NAME = {F32: "f32", F16: "f16", BF16: "bf16"}
UNFUSED, PAIRS, BLOCK, SEGMENTS = 1, 2, 3, 4  # pkg.RB_VARIANT_*
D135 = (1, 3, 5)


def _case(arith, C, k, dils, variant, tiles=0, nr=0):
    return dict(arith=arith, C=C, k=k, dils=tuple(dils), variant=variant, tiles=tiles, nr=nr)


def _cases():
    out = []
    # fp32 pairs: every (taps, dilation) class at C = 32 / 64, the one C = 128 instantiation; fp32 whole blocks, and the same blocks as three chained pairs
    for C in (32, 64):
        for k, dil in ((3, 1), (7, 3), (11, 5)):
            out.append(_case(F32, C, k, (dil,), PAIRS))
    out.append(_case(F32, 128, 3, (1,), PAIRS))
    for C in (32, 64):
        out.append(_case(F32, C, 3, D135, BLOCK))
        out.append(_case(F32, C, 3, D135, PAIRS))
    for arith in (F16, BF16):
        for C in (32, 64):
            for k, dil in ((3, 1), (7, 3), (11, 5)):
                out.append(_case(arith, C, k, (dil,), PAIRS))
        for C, k, dil in ((128, 3, 1), (128, 7, 3), (256, 3, 1), (256, 11, 5)):  # the row-split pairs: both column-tile counts
            for nr in (4, 2):
                out.append(_case(arith, C, k, (dil,), PAIRS, nr=nr))
        # three chained pairs: the 16-bit copy of the stream that a pair writes for the next one (the single pairs above write none)
        for C, k, nr in ((32, 3, 0), (64, 7, 0), (128, 3, 2), (256, 3, 4)):
            out.append(_case(arith, C, k, D135, PAIRS, nr=nr))
        for C, k in ((32, 3), (32, 7), (32, 11), (64, 3), (64, 7), (64, 11), (128, 3)):
            out.append(_case(arith, C, k, D135, BLOCK))
            for tiles in (2, 3):
                out.append(_case(arith, C, k, D135, SEGMENTS, tiles=tiles))
    return out


CASES = _cases()


def case_id(c):
    v = {PAIRS: "pairs", BLOCK: "block", SEGMENTS: "seg%d" % c["tiles"]}[c["variant"]]
    return "%s-C%d-k%d-d%s-%s%s" % (ARITH_NAME[c["arith"]], c["C"], c["k"], "".join(map(str, c["dils"])), v, "-nr%d" % c["nr"] if c["nr"] else "")


def expected_kernel(c):
    """the start of the instantiation's name as the launch-plan tables print it (launch_plan.h: the template arguments that follow are tile shapes the planner owns)"""
    fam = ("rbpair" if c["variant"] == PAIRS else "rbblock") + ("32" if c["arith"] == F32 else "16") + "_kernel<"
    if c["arith"] == F32:
        return fam + ("%d, %d, %d>" % (c["k"], c["dils"][0], c["C"]) if c["variant"] == PAIRS else "%d, " % c["C"])
    if c["variant"] == PAIRS:
        return fam + "%d, %d, %d, %s" % (c["k"], c["dils"][0], c["C"], "%d, " % c["nr"] if c["nr"] else "")
    return fam + "%d, %d, " % (c["k"], c["C"])


def plan_of(pkg, c, T, batch=4):
    pkg.op_set_arith(c["arith"])
    try:
        return pkg.op_resblock_plan(c["C"], c["k"], c["dils"], T, batch=batch, variant=c["variant"], tiles=c["tiles"], nr=c["nr"])
    finally:
        pkg.op_set_arith(F32)


def lengths_of(plan, variant):
    """the lengths of a case, from its kernel's own geometry: around one tile, one tile and its halo, two tiles; for segments also around one and two segments"""
    bo, halo, S = plan["bo"], plan["halo"], plan["segment"]
    Ts = [1, 2, 5, bo - 1, bo, bo + 1, bo + halo + 1, 2 * bo + 3]
    if variant == SEGMENTS:
        Ts += [S - 1, S + 1, 2 * S + 2]
    return sorted(set(Ts))


def ragged(T):
    return [max(1, T - i) for i in range(4)]


# ---- data and the references that the cases of a shape share --------------------------------------------------------------------------------------------------
_DATA, _REF = {}, {}


def data_of(C, k, dils, T):
    """x [4, C, T], accum, weights [ndil, C, C, k] (fp16-valued, as stored models'), biases: one draw per (shape, T), shared by every case of the shape"""
    key = (C, k, dils, T)
    if key not in _DATA:
        rng = np.random.default_rng(R.case_seed(C, C, k, sum(dils), T) + 7)
        x = rng.standard_normal((4, C, T)).astype(np.float32)
        acc = rng.standard_normal((4, C, T)).astype(np.float32)
        w1, w2 = ((rng.standard_normal((len(dils), C, C, k)) / np.sqrt(C * k)).astype(np.float16).astype(np.float32) for _ in range(2))
        b1, b2 = (rng.standard_normal((len(dils), C)).astype(np.float32) for _ in range(2))
        _DATA[key] = (x, acc, w1, b1, w2, b2)
    return _DATA[key]


def run(pkg, c, T, lens, variant=None, accum=False, scale_div=False, x=None, t_stride=None):
    xx, acc, w1, b1, w2, b2 = data_of(c["C"], c["k"], c["dils"], T)
    xx = xx[: len(lens)] if x is None else x
    acc = acc[: len(lens)] if accum else None
    if t_stride is not None:  # the same tensors in rows of t_stride floats, garbage behind t
        pad = lambda a: None if a is None else np.concatenate([a, np.full(a.shape[:2] + (t_stride - T,), 7.5, np.float32)], axis=2)
        xx, acc = pad(xx), pad(acc)
    v = c["variant"] if variant is None else variant
    fused = v == c["variant"]
    return pkg.op_resblock(xx, w1, b1, w2, b2, c["dils"], SLOPE, variant=v, tiles=c["tiles"] if fused else 0, nr=c["nr"] if fused else 0, accum=acc,
                           out_scale=3.0 if scale_div else 1.0 / 3, scale_div=scale_div, lens=lens, t=T)


def composition(pkg, oracle, c, T, lens, accum):
    """the ResBlock as vits_op_conv1d calls; in the 16-bit modes every call is held to the oracle's conv on the same operands (2e-5 of RMS)"""
    x, acc, w1, b1, w2, b2 = data_of(c["C"], c["k"], c["dils"], T)
    y = x
    for p, dil in enumerate(c["dils"]):
        last = p + 1 == len(c["dils"])
        kw1 = dict(dilation=dil, pre_slope=SLOPE, lens=lens)
        kw2 = dict(dilation=1, pre_slope=SLOPE, residual=y, lens=lens)
        if last and accum:
            kw2.update(accum=acc, out_scale=1.0 / 3)
        t = pkg.op_conv1d(y, w1[p], b1[p], **kw1)
        y2 = pkg.op_conv1d(t, w2[p], b2[p], **kw2)
        if c["arith"] != F32 and len(c["dils"]) == 1:
            for got, src, w, b, kw in ((t, y, w1[p], b1[p], kw1), (y2, t, w2[p], b2[p], kw2)):
                want = oracle.conv1d(src, w, b, arith=c["arith"], **kw)
                for r, n in enumerate(lens):
                    assert rel_err(got[r, :, :n], want[r, :, :n]) < 2e-5, ("op_conv1d vs oracle", case_id(c), T, r)
        y = y2
    return y


def unfused(pkg, oracle, c, T, accum):
    """variant 1 on the ragged batch, checked once per (arithmetic, shape, T, accum) against the composition of vits_op_conv1d"""
    key = (c["arith"], c["C"], c["k"], c["dils"], T, accum)
    if key not in _REF:
        lens = ragged(T)
        got = run(pkg, c, T, lens, variant=UNFUSED, accum=accum)
        want = composition(pkg, oracle, c, T, lens, accum)
        for r, n in enumerate(lens):
            assert np.isfinite(got[r, :, :n]).all(), ("variant 1 read behind lens[b]", key, r)
            assert not got[r, :, n:].any(), ("variant 1 wrote past lens[b]", key, r)
            assert np.array_equal(got[r, :, :n], want[r, :, :n]), ("variant 1 != the composition of vits_op_conv1d", key, r, float(np.abs(got[r, :, :n] - want[r, :, :n]).max()))
        _REF[key] = got
    return _REF[key]


def same_bits(label, got, want, lens):
    for r, n in enumerate(lens):
        assert np.isfinite(got[r, :, :n]).all(), (label, r, "a value from behind lens[b] (NaN) was read")
        assert not got[r, :, n:].any(), (label, r, "a column past lens[b] was written")
        if not np.array_equal(got[r, :, :n], want[r, :, :n]):
            bad = np.argwhere(got[r, :, :n] != want[r, :, :n])
            raise AssertionError((label, "row", r, "len", n, "%d values differ; channels %d..%d, columns %d..%d" % (
                len(bad), bad[:, 0].min(), bad[:, 0].max(), bad[:, 1].min(), bad[:, 1].max()), float(np.abs(got[r, :, :n] - want[r, :, :n]).max())))


@pytest.fixture(autouse=True)
def _reset_op_arith(pkg):
    yield
    pkg.op_set_arith(pkg.ARITH_F32)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_fused_kernel_at_every_sequence_end_and_tile_edge(pkg, oracle, c):
    plan = plan_of(pkg, c, 1)
    assert plan["variant"] == c["variant"] and plan["kernel"].startswith(expected_kernel(c)), plan
    if c["variant"] == SEGMENTS:
        assert plan["tiles"] == c["tiles"] and plan["kernel"].endswith("true>") and plan["segment"] == plan["bo"] + (c["tiles"] - 1) * plan["advance"]
    elif c["arith"] != F32 and c["variant"] == BLOCK:
        assert plan["tiles"] == 1 and plan["kernel"].endswith("false>")
    anchor = c["arith"] == F32 and c["variant"] == PAIRS and len(c["dils"]) == 1
    pool, worst = R.EdgePool(), 0.0
    for T in lengths_of(plan, c["variant"]):
        lens = ragged(T)
        pkg.op_set_arith(c["arith"])
        want = unfused(pkg, oracle, c, T, accum=False)
        got = run(pkg, c, T, lens)
        same_bits("%s T %d vs variant 1" % (case_id(c), T), got, want, lens)
        if anchor:
            x, _, w1, b1, w2, b2 = data_of(c["C"], c["k"], c["dils"], T)
            ref, chain, rows = R.pair_reference(x, w1[0], b1[0], w2[0], b2[0], lens, c["dils"][0], SLOPE)
            worst = max(worst, R.hold_to_the_chain("%s T %d" % (case_id(c), T), got, lens, ref, chain, rows))
            pool.add(R.gather_cols(got, lens), ref, chain, rows, R.edge_columns(lens, c["k"], plan["bo"]))
    if anchor:
        print("%s: worst ratio to the chain %.2f overall, %.2f on the edge windows (%d outputs pooled)" % (case_id(c), worst, pool.ratio(), pool.n))
        assert pool.n > 0 and pool.ratio() <= R.FACTOR, (case_id(c), "edge windows", pool.ratio())


def _one_per_kernel_family():
    seen, out = set(), []
    for c in CASES:
        key = (c["arith"], c["variant"])
        if key not in seen and (c["variant"] != SEGMENTS or c["tiles"] == 2):
            seen.add(key)
            out.append(c)
    return out


@pytest.mark.parametrize("c", _one_per_kernel_family(), ids=case_id)
def test_epilogue_forms_rows_and_strides(pkg, oracle, c):
    """accum + out_scale (against variant 1 and the composition), scale_div (among the variants), a row with lens = 0, every row == its batch-1 call, a t_stride larger
    than t and one that is no multiple of 4 — per kernel family and arithmetic, at a length with the sequence end inside a second tile"""
    plan = plan_of(pkg, c, 1)
    T = plan["segment"] + 5
    lens = ragged(T)
    pkg.op_set_arith(c["arith"])
    got = run(pkg, c, T, lens, accum=True)
    same_bits("accum, out_scale", got, unfused(pkg, oracle, c, T, accum=True), lens)
    same_bits("scale_div", run(pkg, c, T, lens, accum=True, scale_div=True), run(pkg, c, T, lens, variant=UNFUSED, accum=True, scale_div=True), lens)
    x = data_of(c["C"], c["k"], c["dils"], T)[0]
    plain = run(pkg, c, T, lens)
    for r, n in enumerate(lens):
        alone = pkg.op_resblock(x[r:r + 1], *data_of(c["C"], c["k"], c["dils"], T)[2:], c["dils"], SLOPE, variant=c["variant"], tiles=c["tiles"], nr=c["nr"], lens=[n], t=n)
        assert np.array_equal(alone[0, :, :n], plain[r, :, :n]), ("a row of the ragged batch != its batch-1 call", r)
    lens0 = [T, 0, T - 2, T - 3]
    got0 = run(pkg, c, T, lens0)
    assert not got0[1].any(), "a row with lens = 0 was written"
    for r in (0, 2, 3):
        assert np.array_equal(got0[r], plain[r]), ("a row next to an empty row changed", r)
    for ts in ((T + 3) // 4 * 4 + 64, T + 1 if (T + 1) % 4 else T + 2):  # rows far longer than t; rows that are no multiple of 4 floats
        wide = run(pkg, c, T, lens, t_stride=ts)
        assert np.array_equal(wide[:, :, :T], plain), ("t_stride %d changed the result" % ts)
        assert not wide[:, :, T:].any()


REFUSALS = [
    # (arith, C, k, dils, variant, tiles, nr, what the message names)
    (F32, 32, 3, (1, 3), BLOCK, 0, 0, "dilations 1, 3, 5"),
    (F16, 32, 3, (1, 3, 2), BLOCK, 0, 0, "dilations 1, 3, 5"),
    (F16, 32, 3, (1, 3, 2), SEGMENTS, 2, 0, "dilations 1, 3, 5"),
    (F32, 128, 7, (3,), PAIRS, 0, 0, "no rbpair32_kernel for C = 128, k = 7"),
    (F32, 32, 3, D135, SEGMENTS, 2, 0, "16-bit modes only"),
    (F32, 32, 7, D135, BLOCK, 0, 0, "no rbblock32_kernel for C = 32, k = 7"),
    (F32, 128, 3, D135, BLOCK, 0, 0, "no rbblock32_kernel for C = 128, k = 3"),
    (BF16, 128, 7, D135, BLOCK, 0, 0, "no rbblock16_kernel for C = 128, k = 7"),
    (F16, 256, 3, D135, SEGMENTS, 2, 0, "no rbblock16_kernel for C = 256, k = 3"),
    (F16, 64, 3, D135, SEGMENTS, 1, 0, "tiles = 1"),
    (F16, 64, 5, (1,), PAIRS, 0, 0, "no rbpair16_kernel for C = 64, k = 5"),
    (F16, 64, 3, (2,), PAIRS, 0, 0, "dilation 2"),
    (F16, 128, 3, (1,), PAIRS, 0, 3, "nr = 3"),
    (F16, 64, 3, (1,), PAIRS, 0, 4, "nr = 4"),
    (F32, 64, 3, (1,), PAIRS, 0, 2, "nr = 2"),
    (F16, 96, 3, (1,), PAIRS, 0, 0, "no rbpair16_kernel for C = 96"),
    (F32, 48, 3, (1,), UNFUSED, 0, 0, "channels = 48"),
    (F32, 32, 4, (1,), UNFUSED, 0, 0, "k = 4"),
    (3, 128, 3, (1,), UNFUSED, 0, 0, "vits_op_resblock_pair"),
    (F32, 32, 3, (1,), 5, 0, 0, "variant 5"),
]


def refusal_id(r):
    return "%s-C%d-k%d-d%s-v%d-t%d-nr%d" % (ARITH_NAME.get(r[0], "split"), r[1], r[2], "".join(map(str, r[3])), r[4], r[5], r[6])


def check_refusal(pkg, r, run_op):
    arith, C, k, dils, variant, tiles, nr, cause = r
    pkg.op_set_arith(arith)
    try:
        with pytest.raises(pkg.VitsError) as e:
            pkg.op_resblock_plan(C, k, dils, 40, batch=2, variant=variant, tiles=tiles, nr=nr)
        assert "vits_op_resblock" in str(e.value) and cause in str(e.value), str(e.value)
        if run_op:
            z = np.zeros((2, C, 40), np.float32)
            w = np.zeros((len(dils), C, C, k), np.float32)
            b = np.zeros((len(dils), C), np.float32)
            with pytest.raises(pkg.VitsError) as e2:
                pkg.op_resblock(z, w, b, w, b, dils, SLOPE, variant=variant, tiles=tiles, nr=nr, lens=[40, 33])
            assert str(e2.value) == str(e.value)
    finally:
        pkg.op_set_arith(F32)


@pytest.mark.parametrize("r", REFUSALS, ids=refusal_id)
def test_refusals_name_their_cause_and_never_fall_back(pkg, r):
    check_refusal(pkg, r, run_op=True)


def test_the_planners_choice_is_one_of_the_forced_variants_bit_for_bit(pkg, oracle):
    """variant 0 resolves as the engine's schedule does and runs the same kernels: fp32 k = 3 at C = 32 the whole block, k = 7 pairs, C = 256 two launches per pair;
    16-bit C = 64, k = 11 on a small grid three fused pairs (the whole-ResBlock kernel only in segments)"""
    for arith, C, k, want in ((F32, 32, 3, BLOCK), (F32, 64, 7, PAIRS), (F32, 256, 3, UNFUSED), (F16, 32, 7, BLOCK), (F16, 64, 11, PAIRS), (BF16, 128, 3, BLOCK)):
        c = _case(arith, C, k, D135, 0)
        plan = plan_of(pkg, c, 77)
        assert plan["variant"] == want, (arith, C, k, plan)
        pkg.op_set_arith(arith)
        lens = ragged(77)
        same_bits("variant 0", run(pkg, c, 77, lens), unfused(pkg, oracle, c, 77, accum=False), lens)
