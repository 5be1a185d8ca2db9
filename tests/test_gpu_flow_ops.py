"""The flow's fused kernels at operator level (wavenet32_kernel, wavenet16_kernel with one and two column tiles per wave, flow_couple16_kernel on its 16-frame and
both 48-frame tiles, through vits_op_flow_coupling), on inputs no whole model produces: a model runs wavenet32_kernel only on grids of 384 blocks and more, picks
the coupling kernel's tile by grid size and knobs, puts sequence ends wherever its predicted durations land, never saturates a gate, always carries the same data
in both channel placements and its own speaker table, and never has a NaN behind lens[b].

Every case of CASES names one kernel (variant, ncw, nct); vits_op_flow_coupling_plan says which instantiation that is, its block width `bo` and halo, and the
lengths are derived from those per case (lengths_of). The batch is lens = [T, T - 1, T - 2, T - 3] (clipped at 1). Data: tests/flow_ref.py (fp16-valued weights
scaled by 1 / sqrt(fan_in), biases 0.1 sigma, a three-row speaker table with bias_rows = [2, 0, 1, 2]; per length a unit-variance draw and a "hot" draw with
x0 x 4 so that gates saturate).

What is asserted:
  * the plan query names the kernel that was asked for;
  * bit identity, no tolerance: every fused variant == variant 1 (ten conv launches, as Engine::run_coupling / run_wavenet build them) on every valid column, for
    both draws, both channel placements (`flipped`) and both directions (the post conv as given, and negated); variant 1 == the composition of vits_op_conv1d
    calls in the same arithmetic (pre conv; per layer the gated conv, post_act = 2, and the 1x1 conv with the stacked [h; out] residual; post conv with residual x1);
  * fp32 anchor: variant 2 (wavenet32_kernel) against numpy float64 under the 2x rule of tests/split_ref.py on the UPDATE m = x1' - x1 — overall, per 32-row tile,
    and pooled on the edge windows (the last k - 1 columns of every row, k - 1 columns on each side of every block boundary) — both draws, every length.
    Observed on an MI355X (the tests print every figure): chain error 4.4e-7 to 8.1e-7 of RMS; GPU / chain overall 0.95 to 1.05 (worst: T = 5, hot draw); per
    32-row tile 0.97 to 1.03 where a tile has 8192 outputs (T >= 63; 0.86 to 1.15 on the 128 to 448 outputs of T = 1, 2, 5, where it is noise and not asserted);
    pooled over every length and both draws: 1.00 on each 32-row tile, 1.00 on the edge windows (28224 outputs);
  * 16-bit anchor: each vits_op_conv1d call of the composition against the oracle's conv in the same arithmetic on the same operands, 2e-5 of RMS (the bound of
    tests/test_gpu_arith16.py and tests/test_gpu_resblock_ops.py), at one length per arithmetic with the sequence end inside a second block. (No rms-ratio rule
    for a fused 16-bit layer: rounding flips of the 16-bit intermediates dominate the ratio of two accumulation orders, as the ResBlock tests measured.)
  * hygiene, per kernel family and arithmetic at T = bo + 5: results finite, x0 bit-unchanged, nothing written past lens[b] (the op stages NaNs there and returns
    them), a lens = 0 row untouched and its neighbours unchanged, every row == its batch-1 call, a t_stride far larger than t and one that is no multiple of 4
    give the same bits, bias_rows == a call whose single-row table holds that utterance's row;
  * refusals name their cause, from the plan query and from the op alike, and never fall back.
tests/test_flow_op_host.py checks this file's own case table and lengths on the CPU."""
import numpy as np
import pytest

import flow_ref as FR
import split_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu
F32, BF16, F16 = 0, 1, 2  # pkg.ARITH_*
ARITH_NAME = {F32: "f32", F16: "f16", BF16: "bf16"}
UNFUSED, WAVENET, COUPLING = 1, 2, 3  # pkg.FLOW_VARIANT_*
H, HALF, K, LAYERS = FR.H, FR.HALF, FR.K, FR.LAYERS
NAN_BITS = 0xFFFFFFFF  # what the op stages behind lens[b]


def _case(arith, variant, ncw=0, nct=0):
    return dict(arith=arith, variant=variant, ncw=ncw, nct=nct)


CASES = [_case(F32, WAVENET)] + [_case(a, v, ncw, nct) for a in (F16, BF16) for v, ncw, nct in
                                 ((WAVENET, 1, 0), (WAVENET, 2, 0), (COUPLING, 1, 1), (COUPLING, 1, 2), (COUPLING, 2, 2))]
# (hot draw, flipped, post conv negated): both draws x both placements x both directions at every length
COMBOS = tuple((hot, flipped, neg) for hot in (False, True) for flipped in (0, 1) for neg in (True, False))


def case_id(c):
    return "%s-%s" % (ARITH_NAME[c["arith"]], {WAVENET: "wavenet-ncw%d" % c["ncw"], COUPLING: "couple-%dx%d" % (c["ncw"], c["nct"])}[c["variant"]])


def expected_kernel(c):
    """the instantiation's name as the launch-plan tables print it (the 16-bit rows of the tables are the f16 kernels: BF = false)"""
    bf = "true" if c["arith"] == BF16 else "false"
    if c["variant"] == WAVENET:
        return "wavenet32_kernel<192, 5>" if c["arith"] == F32 else "wavenet16_kernel<192, 5, %s, %d>" % (bf, c["ncw"])
    return "flow_couple16_kernel<%s, %d, %d>" % (bf, c["ncw"], c["nct"])


def plan_of(pkg, c, T, batch=4, **shape):
    pkg.op_set_arith(c["arith"])
    try:
        return pkg.op_flow_coupling_plan(T, batch=batch, variant=c["variant"], ncw=c["ncw"], nct=c["nct"], **shape)
    finally:
        pkg.op_set_arith(F32)


def lengths_of(plan):
    """the lengths of a case, from its kernel's own geometry: the shortest, around one block, one block and its halo, into a third block"""
    bo, halo = plan["bo"], plan["halo"]
    return sorted({1, 2, 5, bo - 1, bo, bo + 1, bo + halo + 1, 2 * bo + 3})


def ragged(T):
    return [max(1, T - i) for i in range(4)]


# ---- data and results that the cases share --------------------------------------------------------------------------------------------------------------------
_W, _X, _REF = [], {}, {}


def weights():
    if not _W:
        _W.append(FR.make_weights())
    return _W[0]


def inputs(T, hot):
    if (T, hot) not in _X:
        _X[T, hot] = FR.make_inputs(T, hot)
    return _X[T, hot]


def run(pkg, c, z, lens, flipped, neg, variant=None, t=None, bias_rows=FR.BIAS_ROWS, b_in=None):
    W = weights()
    v = c["variant"] if variant is None else variant
    fused = v == c["variant"]
    sign = np.float32(-1 if neg else 1)
    return pkg.op_flow_coupling(z, W["w_pre"], W["b_pre"], W["w_in"], W["b_in"] if b_in is None else b_in, W["w_rs"], W["b_rs"], sign * W["w_post"],
                                sign * W["b_post"], flipped=flipped, variant=v, ncw=c["ncw"] if fused else 0, nct=c["nct"] if fused else 0,
                                bias_rows=None if bias_rows is None else bias_rows[: len(lens)], lens=lens, t=t)


def composition(pkg, x0, x1, lens, neg, oracle=None, arith=F32):
    """the coupling layer as vits_op_conv1d calls (the speaker rows: one gated conv per table row, every utterance takes its own); with an oracle, every call is
    held to the oracle's conv in the same arithmetic on the same operands (2e-5 of RMS)"""
    W = weights()

    def conv(x, w, b, **kw):
        got = pkg.op_conv1d(x, w, b, lens=lens, **kw)
        if oracle is not None:
            want = oracle.conv1d(x, w, b, lens=lens, arith=arith, **kw)
            for r, n in enumerate(lens):
                assert rel_err(got[r, :, :n], want[r, :, :n]) < 2e-5, ("op_conv1d vs oracle", ARITH_NAME[arith], w.shape, r)
        return got

    h = conv(x0, W["w_pre"], W["b_pre"])
    out = np.zeros_like(h)
    for l in range(LAYERS):
        per_row = {row: conv(h, W["w_in"][l], W["b_in"][row, l], post_act=2) for row in sorted(set(FR.BIAS_ROWS))}
        a = np.stack([per_row[FR.BIAS_ROWS[b]][b] for b in range(len(lens))])
        if l + 1 < LAYERS:
            ho = conv(a, W["w_rs"][l], W["b_rs"][l], residual=np.concatenate([h, out], axis=1))
            h, out = ho[:, :H], ho[:, H:]
        else:
            out = conv(a, W["w_rs"][l], W["b_rs"][l], residual=out)
    sign = np.float32(-1 if neg else 1)
    return conv(out, sign * W["w_post"], sign * W["b_post"], residual=x1)


def check_result(label, got, z, lens, flipped):
    """what every result must satisfy: valid columns finite, x0 the input's bits, the staged NaNs behind lens[b] untouched in both halves"""
    gx0, gx1 = FR.halves(got, flipped)
    zx0, _ = FR.halves(z, flipped)
    for r, n in enumerate(lens):
        assert np.isfinite(gx1[r, :, :n]).all(), (label, r, "a value from behind lens[b] (NaN) was read")
        assert np.array_equal(gx0[r, :, :n], zx0[r, :, :n]), (label, r, "x0 changed")
        assert (got[r, :, n:].view(np.uint32) == NAN_BITS).all(), (label, r, "a column past lens[b] was written")
    return gx1


def same_bits(label, got, want, lens):
    for r, n in enumerate(lens):
        if not np.array_equal(got[r, :, :n], want[r, :, :n]):
            bad = np.argwhere(got[r, :, :n] != want[r, :, :n])
            raise AssertionError((label, "row", r, "len", n, "%d values differ; channels %d..%d, columns %d..%d" % (
                len(bad), bad[:, 0].min(), bad[:, 0].max(), bad[:, 1].min(), bad[:, 1].max()), float(np.abs(got[r, :, :n] - want[r, :, :n]).max())))


def unfused(pkg, arith, T, combo, compose):
    """x1' of variant 1 on the ragged batch; with `compose` checked once per (arithmetic, T, combo) against the composition of vits_op_conv1d"""
    key = (arith, T, combo)
    hot, flipped, neg = combo
    lens = ragged(T)
    x0, x1 = inputs(T, hot)
    if key not in _REF:
        z = FR.place(x0, x1, flipped)
        _REF[key] = [check_result("variant 1 %s" % (key,), run(pkg, _case(arith, UNFUSED), z, lens, flipped, neg), z, lens, flipped), False]
    if compose and not _REF[key][1]:
        same_bits("variant 1 != the composition of vits_op_conv1d %s" % (key,), _REF[key][0], composition(pkg, x0, x1, lens, neg), lens)
        _REF[key][1] = True
    return _REF[key][0]


@pytest.fixture(autouse=True)
def _reset_op_arith(pkg):
    yield
    pkg.op_set_arith(pkg.ARITH_F32)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_fused_kernel_at_every_sequence_end_and_block_edge(pkg, c):
    plan = plan_of(pkg, c, 1)
    assert plan["variant"] == c["variant"] and plan["kernel"] == expected_kernel(c), plan
    pkg.op_set_arith(c["arith"])
    for T in lengths_of(plan):
        lens = ragged(T)
        for combo in COMBOS:
            hot, flipped, neg = combo
            want = unfused(pkg, c["arith"], T, combo, compose=True)
            z = FR.place(*inputs(T, hot), flipped)
            label = "%s T %d hot %d flipped %d negated %d" % (case_id(c), T, hot, flipped, neg)
            same_bits(label + " vs variant 1", check_result(label, run(pkg, c, z, lens, flipped, neg), z, lens, flipped), want, lens)


# ---- fp32: wavenet32_kernel against float64 ---------------------------------------------------------------------------------------------------------------------
_WORST = {"overall": 0.0}
_EDGES = R.EdgePool()
_TILES = [R.EdgePool() for _ in range(HALF // 32)]
FP32_LENGTHS = (1, 2, 5, 63, 64, 65, 67, 131)  # lengths_of(wavenet32_kernel's plan): checked against the plan in the test


@pytest.mark.parametrize("T", FP32_LENGTHS)
def test_fp32_fused_wavenet_layers_against_float64(pkg, T):
    """The 2x rule on m = x1' - x1, both draws: overall, and per 32-row tile where a tile has split_ref.MIN_ELEMS outputs (below that a tile's rms is noise; every
    length enters the pooled tiles and edge windows of the next test)."""
    c = CASES[0]
    plan = plan_of(pkg, c, 1)
    assert tuple(lengths_of(plan)) == FP32_LENGTHS and plan["kernel"] == "wavenet32_kernel<192, 5>"
    lens = ragged(T)
    W = weights()
    mask = R.edge_columns(lens, K, plan["bo"])
    every = np.ones(mask.size, bool)
    for hot in (False, True):
        x0, x1 = inputs(T, hot)
        z = FR.place(x0, x1, 0)
        got = check_result("fp32 T %d hot %d" % (T, hot), run(pkg, c, z, lens, 0, False), z, lens, 0)
        m64, m32, x1c = FR.layer_reference(x0, x1, W, lens, FR.BIAS_ROWS)
        m = FR.update_of(got, x1c, lens)
        g, ch = FR.ratios(m, m64, m32)
        tiles = [R.rms_err(m[32 * i:32 * i + 32], m64[32 * i:32 * i + 32])[0] / ch for i in range(HALF // 32)]
        print("fp32 T %d hot %d: %d outputs: gpu rms %.2e, chain rms %.2e of RMS: ratio %.2f; per 32-row tile %s" % (
            T, hot, m.size, g, ch, g / ch, " ".join("%.2f" % t for t in tiles)))
        _WORST["overall"] = max(_WORST["overall"], g / ch)
        _EDGES.add(m, m64, m32, np.arange(HALF), mask)
        for i, pool in enumerate(_TILES):
            pool.add(m[32 * i:32 * i + 32], m64[32 * i:32 * i + 32], m32[32 * i:32 * i + 32], np.arange(32), every)
        assert g <= FR.FACTOR * ch, ("overall", T, hot, g, ch)
        if 32 * m.shape[1] >= R.MIN_ELEMS:
            assert max(tiles) <= FR.FACTOR, ("row tile", T, hot, tiles)


def test_fp32_edge_windows_and_row_tiles_pooled_over_every_length(pkg):
    """The rule on the edge windows alone and on each 32-row tile alone, squared errors pooled over every length and both draws (the per-length tests above fill
    the pools; run alone, this test runs them first)."""
    if _EDGES.n == 0:
        for T in FP32_LENGTHS:
            test_fp32_fused_wavenet_layers_against_float64(pkg, T)
    tiles = [p.ratio() for p in _TILES]
    print("fp32 wavenet32_kernel: worst ratio to the chain %.2f overall; pooled: %s per 32-row tile, %.2f on the edge windows (%d outputs)" % (
        _WORST["overall"], " ".join("%.2f" % t for t in tiles), _EDGES.ratio(), _EDGES.n))
    assert _EDGES.n > 0 and _EDGES.ratio() <= FR.FACTOR, ("edge windows", _EDGES.ratio())
    assert max(tiles) <= FR.FACTOR, ("row tiles", tiles)


# ---- 16-bit: every conv of the composition against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", [F16, BF16], ids=["f16", "bf16"])
def test_each_conv_of_the_composition_against_the_oracle(pkg, oracle, arith):
    T = 64 + 5  # the sequence end inside the second block of the 64- and the 48-frame kernels
    pkg.op_set_arith(arith)
    combo = (False, 0, True)
    lens = ragged(T)
    x0, x1 = inputs(T, False)
    same_bits("variant 1 != the composition", unfused(pkg, arith, T, combo, compose=False), composition(pkg, x0, x1, lens, True, oracle, arith), lens)


# ---- hygiene ----------------------------------------------------------------------------------------------------------------------------------------------------
def _one_per_kernel_family():
    seen, out = set(), []
    for c in CASES:
        key = (c["arith"], c["variant"], c["nct"])  # the 16- and the 48-frame tile of the coupling kernel count as two families
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


@pytest.mark.parametrize("c", _one_per_kernel_family(), ids=case_id)
def test_rows_strides_empty_rows_and_speaker_rows(pkg, c):
    plan = plan_of(pkg, c, 1)
    T = plan["bo"] + 5
    lens = ragged(T)
    hot, flipped, neg = False, 1, True
    x0, x1 = inputs(T, hot)
    z = FR.place(x0, x1, flipped)
    W = weights()
    pkg.op_set_arith(c["arith"])
    plain_z = run(pkg, c, z, lens, flipped, neg)
    plain = check_result("plain", plain_z, z, lens, flipped)
    # every row == its batch-1 call, with that utterance's table row as a single-row table and no bias_rows
    for r, n in enumerate(lens):
        alone = run(pkg, c, z[r:r + 1, :, :n], [n], flipped, neg, bias_rows=None, b_in=W["b_in"][FR.BIAS_ROWS[r]][None])
        assert np.array_equal(alone[0], plain_z[r, :, :n]), ("a row of the ragged batch != its batch-1 call", r)
    # bias_rows == a call whose single-row table holds the row (utterances 0 and 3 share row 2)
    only2 = run(pkg, c, z, lens, flipped, neg, bias_rows=None, b_in=W["b_in"][2][None])
    for r in (0, 3):
        assert np.array_equal(FR.halves(only2, flipped)[1][r, :, :lens[r]], plain[r, :, :lens[r]]), ("bias_rows", r)
    assert not np.array_equal(FR.halves(only2, flipped)[1][1, :, :lens[1]], plain[1, :, :lens[1]]), "the speaker rows make no difference: the check is void"
    # a row with lens = 0 comes back as staged, its neighbours with the same bits
    lens0 = [T, 0, T - 2, T - 3]
    got0 = run(pkg, c, z, lens0, flipped, neg)
    check_result("lens 0", got0, z, lens0, flipped)
    assert (got0[1].view(np.uint32) == NAN_BITS).all(), "a row with lens = 0 was written"
    for r in (0, 2, 3):
        assert np.array_equal(got0[r, :, :lens0[r]], plain_z[r, :, :lens0[r]]), ("a row next to an empty row changed", r)
    # rows far longer than t; rows that are no multiple of 4 floats: garbage behind t stays where it is
    for ts in ((T + 3) // 4 * 4 + 64, T + 1 if (T + 1) % 4 else T + 2):
        zw = np.concatenate([z, np.full(z.shape[:2] + (ts - T,), 7.5, np.float32)], axis=2)
        wide = run(pkg, c, zw, lens, flipped, neg, t=T)
        assert np.array_equal(wide[:, :, :T].view(np.uint32), plain_z.view(np.uint32)), ("t_stride %d changed the result" % ts)
        assert (wide[:, :, T:] == 7.5).all(), "columns behind t were written"


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
REFUSALS = [
    # (arith, shape overrides, variant, ncw, nct, what the message names)
    (F32, {}, COUPLING, 0, 0, "16-bit modes only"),
    (F32, {}, COUPLING, 1, 1, "16-bit modes only"),
    (F32, {}, WAVENET, 1, 0, "wavenet32_kernel has one form"),
    (F32, dict(hidden=128), WAVENET, 0, 0, "no wavenet32_kernel for hidden = 128"),
    (F32, dict(k=3), WAVENET, 0, 0, "no wavenet32_kernel for k = 3"),
    (F32, dict(rate=2), WAVENET, 0, 0, "no wavenet32_kernel for rate = 2"),
    (F16, dict(hidden=256), WAVENET, 1, 0, "no wavenet16_kernel for hidden = 256"),
    (BF16, dict(k=7), WAVENET, 2, 0, "no wavenet16_kernel for k = 7"),
    (F16, {}, WAVENET, 3, 0, "(ncw, nct) = (3, 0): no such wavenet16_kernel"),
    (F16, {}, WAVENET, 1, 2, "variant 2 has no nct"),
    (F16, dict(hidden=128), COUPLING, 0, 0, "no flow_couple16_kernel for hidden = 128"),
    (F16, dict(half=64), COUPLING, 1, 1, "no flow_couple16_kernel for half = 64"),
    (BF16, dict(k=3), COUPLING, 2, 2, "no flow_couple16_kernel for k = 3"),
    (F16, dict(rate=2), COUPLING, 0, 0, "no flow_couple16_kernel for rate = 2"),
    (BF16, dict(layers=3), COUPLING, 1, 2, "no flow_couple16_kernel for layers = 3"),
    (F16, {}, COUPLING, 2, 1, "(ncw, nct) = (2, 1): no such flow_couple16_kernel"),
    (BF16, {}, COUPLING, 1, 3, "(ncw, nct) = (1, 3): no such flow_couple16_kernel"),
    (F16, {}, COUPLING, 0, 2, "(ncw, nct) = (0, 2): no such flow_couple16_kernel"),
    (F16, {}, UNFUSED, 1, 0, "variant 1 has no tile to choose"),
    (F32, dict(hidden=100), UNFUSED, 0, 0, "hidden = 100"),
    (F32, dict(k=4), UNFUSED, 0, 0, "k = 4"),
    (3, {}, UNFUSED, 0, 0, "the split arithmetic has no flow kernels"),
    (3, {}, WAVENET, 0, 0, "the split arithmetic has no flow kernels"),
    (F32, {}, 4, 0, 0, "variant 4"),
]


def refusal_id(r):
    return "%s-%s-v%d-%dx%d" % (ARITH_NAME.get(r[0], "split"), "-".join("%s%d" % kv for kv in sorted(r[1].items())) or "std", r[2], r[3], r[4])


def check_refusal(pkg, r):
    arith, shape, variant, ncw, nct, cause = r
    s = dict(hidden=H, half=HALF, k=K, layers=LAYERS, rate=1)
    s.update(shape)
    pkg.op_set_arith(arith)
    try:
        with pytest.raises(pkg.VitsError) as e:
            pkg.op_flow_coupling_plan(40, batch=2, variant=variant, ncw=ncw, nct=nct, **s)
        assert "vits_op_flow_coupling" in str(e.value) and cause in str(e.value), str(e.value)
        # the op itself: the same message, before any device call (this runs on a machine without a GPU as well)
        Hh, hf, L = s["hidden"], s["half"], s["layers"]
        z = np.zeros((2, 2 * hf, 40), np.float32)
        with pytest.raises(pkg.VitsError) as e2:
            pkg.op_flow_coupling(z, np.zeros((Hh, hf, 1)), np.zeros(Hh), np.zeros((L, 2 * Hh, Hh, s["k"])), np.zeros((1, L, 2 * Hh)), np.zeros((2 * L - 1) * Hh * Hh),
                                 np.zeros((2 * L - 1) * Hh), np.zeros((hf, Hh, 1)), np.zeros(hf), rate=s["rate"], variant=variant, ncw=ncw, nct=nct, lens=[40, 33])
        assert str(e2.value) == str(e.value)
    finally:
        pkg.op_set_arith(F32)


@pytest.mark.parametrize("r", REFUSALS, ids=refusal_id)
def test_refusals_name_their_cause_and_never_fall_back(pkg, r):
    check_refusal(pkg, r)


def test_the_planners_choice_is_one_of_the_forced_variants_bit_for_bit(pkg):
    """variant 0 resolves as the engine does: fp32 on this grid ten launches (the fused layers need 384 blocks), the 16-bit modes the coupling kernel on the tile
    the grid rule picks"""
    T, combo = 77, (False, 0, True)
    lens = ragged(T)
    z = FR.place(*inputs(T, False), 0)
    for arith, want in ((F32, UNFUSED), (F16, COUPLING), (BF16, COUPLING)):
        c = _case(arith, 0)
        assert plan_of(pkg, c, T)["variant"] == want
        pkg.op_set_arith(arith)
        same_bits("variant 0", check_result("variant 0", run(pkg, c, z, lens, 0, True), z, lens, 0), unfused(pkg, arith, T, combo, compose=False), lens)
