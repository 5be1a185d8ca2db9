"""The text encoder's LayerNorm kernels at operator level: add_layer_norm_kernel<32 | 64> with every argument its callers pass (vits_op_layer_norm) and LayerNorm
on load in conv_lat16_kernel against the separate launch (vits_op_norm_conv), on inputs no whole model produces: a model normalises 192 or 512 channels on the
32-step tile, with the GELU epilogue and the read-modify-write form only inside the duration predictor's 192 channels, normalises on load only at 192 -> {576, 768,
384} with k in {1, 3} and symmetric padding, and never has anything but zeros behind lens[b].

The batch is lens = [T, T - 1, T - 2, T - 3] clipped at 1; the lengths come from the tile the plan query names (lengths_of). Data: tests/norm_ref.py (a
unit-variance draw and an "offset" draw, mean 50 and sigma 1, where a one-pass variance would lose every digit in fp32).

vits_op_layer_norm, channels in {5, 16, 29, 192, 200, 512} (fewer channels than the sixteen channel groups, one per group, a ragged last round, the twelve-channel
load loop's full step, one step and a tail, three steps) x {plain, residual, GELU, GELU + add_to, GELU table}:
  * the tiles of 32 and of 64 time steps give the same bits, on both draws, at every length;
  * the 2x rule of tests/split_ref.py against float64 (rms error <= 2 x the sequential fp32 restatement's), per length where a case has 2000 outputs and pooled
    over the lengths on the tile edges; with the GELU table the fp16 lookup decides (see tests/test_gpu_attention_ops.py): rms error <= 2^-11 of RMS;
  * add_to == y0 + the write form's bits, one fp32 addition;
  * hygiene: results finite, the staged 0xFF bytes behind lens[b], a lens = 0 row untouched and its neighbours unchanged, every row == its batch-1 call, the old
    vits_op_add_layer_norm == tw 0.
vits_op_norm_conv, (cin, cout, k, pad_left) over cin in {72, 192, 768, 800} x cout in {32, 192, 576} (gridDim.y = 1, 3, 9: one writer row group among several) x
k in {1, 3, 5} x pad_left in {0, (k - 1) / 2, k - 1}, lengths {1, 2, 15, 16, 17, 31, 33, 40} at batch 1 and at the ragged batch 4, every plan TILE_LAT16:
  * variant 2 (on load) == variant 1 (LayerNorm launch + conv) bit for bit in y and in ln_out; for cin = 800, beyond the 768 channels whose gamma and beta the
    kernel stages, variant 2 is refused with that condition named and variant 0 runs the two launches;
  * ln_out has every valid column written and nothing behind lens[b] touched (the op stages 0xFF bytes there), y likewise;
  * the engine's pitch and pitch 37 (the element-wise fill; 41 at T = 40, whose rows do not fit 37) give the same bits;
  * variant 1's y == vits_op_conv1d on variant 1's ln_out;
  * ln_out against float64 under the 2x rule.
Observed on an MI355X (the tests print every figure). vits_op_layer_norm: restatement error 5.3e-8 to 1.9e-7 of RMS on the unit draw, 1.7e-6 to 1.9e-5 on the offset
draw (the rounding of the mean, 50, against a sigma of 1); GPU / restatement where asserted 0.36 to 0.98 and 0.11 to 1.09 (sixteen partial sums are more accurate than one
sequential sum), 0.17 to 1.45 on the cases below 2000 outputs (printed only); pooled on the tile edges 0.19 to 1.00; with the GELU table at most 1.8e-4 of RMS against
the bound 4.9e-4 (offset draw, where a hundredth of the entries sits within the fp32 error of an fp16 boundary). vits_op_norm_conv: ln_out's restatement error 7.1e-8 to
3.0e-7 of RMS, GPU / restatement 0.17 to 0.90 where asserted (up to 2.0 below 2000 outputs, printed only), pooled per case 0.30 to 0.77.
tests/test_encoder_op_host.py checks this file's case tables on the CPU."""
import numpy as np
import pytest

import norm_ref as NR
import split_ref as R

pytestmark = pytest.mark.gpu
BATCH = 4
EPS = 1e-5
NAN_BITS = 0xFFFFFFFF
TABLE_BOUND = 2.0 ** -11
CHANNELS = (5, 16, 29, 192, 200, 512)
TWS = (32, 64)
MODES = ("plain", "residual", "gelu", "gelu_add_to", "gelu_table")
LN_CASES = [(C, m) for C in CHANNELS for m in MODES]


def lengths_of(tw):
    return sorted({1, 2, tw - 1, tw, tw + 1, 2 * tw + 3})


LN_LENGTHS = tuple(sorted(set(lengths_of(32)) | set(lengths_of(64))))  # both tiles run every length: bit identity needs them in common


def ragged(T, batch=BATCH):
    return [max(1, T - i) for i in range(batch)]


_TAB = []


def gelu_table():
    if not _TAB:
        _TAB.append(NR.gelu_table())
    return _TAB[0]


def check_result(label, out, lens):
    """valid columns finite, every other element the staged 0xFF bytes"""
    for b, n in enumerate(lens):
        assert np.isfinite(out[b, :, :n]).all(), (label, b, "a valid column is missing, or a value from behind lens[b] (NaN) was read")
        assert (out[b, :, n:].view(np.uint32) == NAN_BITS).all(), (label, b, "a column past lens[b] was written")
    return out


def same_bits(label, got, want, lens):
    for b, n in enumerate(lens):
        if not np.array_equal(got[b, :, :n], want[b, :, :n]):
            bad = np.argwhere(got[b, :, :n] != want[b, :, :n])
            raise AssertionError((label, "row", b, "len", n, "%d values differ; channels %d..%d, columns %d..%d" % (
                len(bad), bad[:, 0].min(), bad[:, 0].max(), bad[:, 1].min(), bad[:, 1].max()), float(np.abs(got[b, :, :n] - want[b, :, :n]).max())))


def ln_kwargs(mode, res, y0):
    """(op_layer_norm's keyword arguments, the references' keyword arguments) of a mode"""
    if mode == "plain":
        return {}, dict(res=None)
    if mode == "residual":
        return dict(residual=res), dict(res=res)
    if mode == "gelu":
        return dict(post_gelu=True), dict(res=None, gelu=True)
    if mode == "gelu_add_to":
        return dict(post_gelu=True, add_to=y0), dict(res=None, gelu=True)
    return dict(post_gelu=True, gelu_tab=gelu_table()), dict(res=None, gelu_tab=gelu_table())


def asserted_ln_lengths(C):
    return [T for T in LN_LENGTHS if C * sum(ragged(T)) >= NR.MIN_OUTPUTS]


@pytest.mark.parametrize("c", LN_CASES, ids=lambda c: "c%d-%s" % c)
def test_layer_norm_both_tiles_same_bits_and_against_float64(pkg, c):
    C, mode = c
    for tw in TWS:
        p = pkg.op_layer_norm_plan(C, 1, batch=BATCH, tw=tw)
        assert p["kernel"] == "add_layer_norm_kernel<%d>" % tw and p["tw"] == tw and set(lengths_of(p["tw"])) <= set(LN_LENGTHS), p
    pool, asserted = R.EdgePool(), 0
    for T in LN_LENGTHS:
        lens = ragged(T)
        mask = NR.edge_columns(lens, 32) | NR.edge_columns(lens, 64)
        for offset in (False, True):
            x, res, y0, gamma, beta = NR.make_case(C, T, BATCH, offset)
            kw, rkw = ln_kwargs(mode, res, y0)
            label = "c%d %s T %d offset %d" % (C, mode, T, offset)
            got = check_result(label, pkg.op_layer_norm(x, gamma, beta, eps=EPS, tw=32, lens=lens, **kw), lens)
            same_bits(label + ": tw 64 vs tw 32", check_result(label, pkg.op_layer_norm(x, gamma, beta, eps=EPS, tw=64, lens=lens, **kw), lens), got, lens)
            ref, chain = NR.reference64(x, gamma=gamma, beta=beta, eps=EPS, lens=lens, **rkw), NR.chain32(x, gamma=gamma, beta=beta, eps=EPS, lens=lens, **rkw)
            if mode == "gelu_add_to":
                write = pkg.op_layer_norm(x, gamma, beta, eps=EPS, tw=32, lens=lens, post_gelu=True)
                same_bits(label + ": add_to vs y0 + the write form", got, (y0 + write).astype(np.float32), lens)
                y0c = R.gather_cols(y0, lens)
                ref, chain = ref + y0c.astype(np.float64), (y0c + chain).astype(np.float32)
            cols = R.gather_cols(got, lens)
            g_rms, g_max = R.rms_err(cols, ref)
            c_rms, c_max = R.rms_err(chain, ref)
            print("%s: %d outputs: gpu rms %.2e max %.2e of RMS; restatement rms %.2e max %.2e; ratio %.2f" % (label, cols.size, g_rms, g_max, c_rms, c_max, g_rms / (c_rms + 1e-300)))
            if mode == "gelu_table":
                assert g_rms <= TABLE_BOUND, (label, g_rms)
                continue
            pool.add(cols, ref, chain, np.arange(C), mask)
            if cols.size >= NR.MIN_OUTPUTS:
                assert g_rms <= NR.FACTOR * c_rms, (label, g_rms, c_rms)
                asserted += 1
    if mode != "gelu_table":
        assert asserted == 2 * len(asserted_ln_lengths(C)) and asserted >= 2, asserted
        print("c%d %s pooled over every length and both draws on the tile edges: %.2f (%d outputs)" % (C, mode, pool.ratio(), pool.n))
        if pool.n >= NR.MIN_OUTPUTS:
            assert pool.ratio() <= NR.FACTOR, ("tile edges", pool.ratio())


@pytest.mark.parametrize("h", [(C, tw) for C in (29, 192) for tw in TWS], ids=lambda h: "c%d-tw%d" % h)
def test_layer_norm_rows_empty_rows_and_the_old_entry_point(pkg, h):
    C, tw = h
    T = tw + 5
    lens = ragged(T)
    x, res, y0, gamma, beta = NR.make_case(C, T, BATCH, False)
    kw = dict(eps=EPS, tw=tw, residual=res, post_gelu=True)
    plain = check_result("plain", pkg.op_layer_norm(x, gamma, beta, lens=lens, **kw), lens)
    for b, n in enumerate(lens):
        alone = pkg.op_layer_norm(x[b:b + 1, :, :n], gamma, beta, lens=[n], eps=EPS, tw=tw, residual=res[b:b + 1, :, :n], post_gelu=True)
        assert np.array_equal(alone[0], plain[b, :, :n]), ("a row of the ragged batch != its batch-1 call", b)
    lens0 = [T, 0, T - 2, T - 3]
    got0 = check_result("lens 0", pkg.op_layer_norm(x, gamma, beta, lens=lens0, **kw), lens0)
    assert (got0[1].view(np.uint32) == NAN_BITS).all(), "a row with lens = 0 was written"
    for b in (0, 2, 3):
        assert np.array_equal(got0[b, :, :lens0[b]], plain[b, :, :lens0[b]]), ("a row next to an empty row changed", b)
    # add_to leaves what lies behind lens[b] alone as well: the staged bytes come back
    added = check_result("add_to", pkg.op_layer_norm(x, gamma, beta, lens=lens, add_to=y0, **kw), lens)
    same_bits("add_to", added, (y0 + plain).astype(np.float32), lens)
    # the old entry point (no lens, no GELU): the bits of tw 0, which is the tile of 32
    old = pkg.op_add_layer_norm(x, res, gamma, beta, eps=EPS)
    new = pkg.op_layer_norm(x, gamma, beta, residual=res, eps=EPS, tw=0)
    assert pkg.op_layer_norm_plan(C, T, batch=BATCH)["tw"] == 32
    assert np.array_equal(old.view(np.uint32), new.view(np.uint32))
    assert np.array_equal(new, pkg.op_layer_norm(x, gamma, beta, residual=res, eps=EPS, tw=tw))


# ---- LayerNorm on load ------------------------------------------------------------------------------------------------------------------------------------------
NC_CIN, NC_COUT, NC_K = (72, 192, 768, 800), (32, 192, 576), (1, 3, 5)
NC_LENGTHS = (1, 2, 15, 16, 17, 31, 33, 40)
NC_CASES = [(cin, cout, k) for cin in NC_CIN for cout in NC_COUT for k in NC_K]
LN_ON_LOAD_MAX_CIN = 768


def odd_pitch(T):
    """a device pitch that is no multiple of 4 (the element-wise fill): 37, and 41 where the rows of T = 40 do not fit 37"""
    return 37 if T <= 37 else 41


def pads_of(k):
    return sorted({0, (k - 1) // 2, k - 1})


def nc_data(cin, cout, k, T, B):
    rng = np.random.default_rng(((cin * 1009 + cout) * 131 + k) * 4099 + T * 8 + B)
    x = rng.standard_normal((B, cin, T)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, k)) / np.sqrt(cin * k)).astype(np.float16).astype(np.float32)
    bias = rng.standard_normal(cout).astype(np.float32)
    res = rng.standard_normal((B, cout, T)).astype(np.float32)
    gamma = (1 + 0.1 * rng.standard_normal(cin)).astype(np.float32)
    beta = (0.5 * rng.standard_normal(cin)).astype(np.float32)
    return x, w, bias, res, gamma, beta


@pytest.mark.parametrize("c", NC_CASES, ids=lambda c: "cin%d-cout%d-k%d" % c)
def test_layer_norm_on_load_equals_the_separate_launch(pkg, c):
    cin, cout, k = c
    post_act = 1 if k == 3 else 0      # the FFN conv's relu
    with_res = cout == 192             # (the op takes a residual; the engine's convs of a norm have none)
    on_load = cin <= LN_ON_LOAD_MAX_CIN
    pool = R.EdgePool()
    for pad in pads_of(k):
        for T in NC_LENGTHS:
            for B in (1, BATCH):
                lens = ragged(T, B)
                label = "cin %d cout %d k %d pad %d T %d batch %d" % (cin, cout, k, pad, T, B)
                plan = pkg.op_norm_conv_plan(cin, cout, k, T, batch=B, pad_left=pad, post_act=post_act, variant=1)
                assert plan["tile"] == "TILE_LAT16" and plan["launches"] == 2 and plan["ln_ok"] == on_load, (label, plan)
                auto = pkg.op_norm_conv_plan(cin, cout, k, T, batch=B, pad_left=pad, post_act=post_act)
                assert auto["variant"] == (2 if on_load else 1), (label, auto)
                x, w, bias, res, gamma, beta = nc_data(cin, cout, k, T, B)
                kw = dict(bias=bias, residual=res if with_res else None, pad_left=pad, post_act=post_act, eps=EPS, lens=lens)
                y1, ln1 = pkg.op_norm_conv(x, gamma, beta, w, variant=1, **kw)
                check_result(label + " variant 1 y", y1, lens), check_result(label + " variant 1 ln_out", ln1, lens)
                if on_load:
                    p2 = pkg.op_norm_conv_plan(cin, cout, k, T, batch=B, pad_left=pad, post_act=post_act, variant=2)
                    assert p2["tile"] == "TILE_LAT16" and p2["launches"] == 1 and p2["grid"] == ((T + 15) // 16, (cout + 63) // 64, B), (label, p2)
                    for pitch in (0, odd_pitch(T)):
                        y2, ln2 = pkg.op_norm_conv(x, gamma, beta, w, variant=2, pitch=pitch, **kw)
                        check_result(label + " variant 2 y", y2, lens), check_result(label + " variant 2 ln_out", ln2, lens)
                        same_bits(label + " pitch %d: y, variant 2 vs 1" % pitch, y2, y1, lens)
                        same_bits(label + " pitch %d: ln_out, variant 2 vs 1" % pitch, ln2, ln1, lens)
                else:
                    with pytest.raises(pkg.VitsError) as e:
                        pkg.op_norm_conv(x, gamma, beta, w, variant=2, **kw)
                    assert "c_in > 768" in str(e.value) and "conv_ln_on_load_ok refuses" in str(e.value), str(e.value)
                    y0_, ln0_ = pkg.op_norm_conv(x, gamma, beta, w, variant=0, **kw)
                    same_bits(label + ": variant 0 falls back to the two launches", y0_, y1, lens), same_bits(label + ": variant 0 ln_out", ln0_, ln1, lens)
                y1p, ln1p = pkg.op_norm_conv(x, gamma, beta, w, variant=1, pitch=odd_pitch(T), **kw)
                same_bits(label + ": y, variant 1, odd pitch", y1p, y1, lens), same_bits(label + ": ln_out, variant 1, odd pitch", ln1p, ln1, lens)
                conv = pkg.op_conv1d(np.where(np.isfinite(ln1), ln1, np.float32(0)), w, bias, pad_left=pad, post_act=post_act, residual=res if with_res else None, lens=lens)
                same_bits(label + ": variant 1's conv vs vits_op_conv1d on its ln_out", y1, conv, lens)
                if pad == pads_of(k)[0]:  # (ln_out does not depend on the padding)
                    ref, chain = NR.reference64(x, None, gamma, beta, EPS, lens), NR.chain32(x, None, gamma, beta, EPS, lens)
                    cols = R.gather_cols(ln1, lens)
                    g_rms, _ = R.rms_err(cols, ref)
                    c_rms, _ = R.rms_err(chain, ref)
                    print("%s: ln_out, %d outputs: gpu rms %.2e, restatement rms %.2e of RMS: ratio %.2f" % (label, cols.size, g_rms, c_rms, g_rms / c_rms))
                    pool.add(cols, ref, chain, np.arange(cin), np.ones(cols.shape[1], bool))
                    if cols.size >= NR.MIN_OUTPUTS:
                        assert g_rms <= NR.FACTOR * c_rms, (label, g_rms, c_rms)
    print("cin %d cout %d k %d: ln_out pooled over every length and batch: %.2f (%d outputs)" % (cin, cout, k, pool.ratio(), pool.n))
    assert pool.n >= NR.MIN_OUTPUTS and pool.ratio() <= NR.FACTOR, pool.ratio()


NC_REFUSALS = [
    # (keyword overrides of (cin 192, cout 192, k 3, t 40, batch 1), what the message names)
    (dict(cin=800, variant=2), "c_in > 768"),
    (dict(cin=1024, k=1, variant=2), "c_in > 768"),
    (dict(batch=64, t=128, variant=2), "the planner's tile is not TILE_LAT16"),
    (dict(k=19, pad_left=9, variant=2), "(k - 1) * dilation > 16"),
    (dict(cin=8, k=3, variant=2), "the layer has no conv_lat16_kernel weights"),
    (dict(pad_left=3), "pad_left = 3"),
    (dict(pad_left=-1), "pad_left = -1"),
    (dict(post_act=2), "post_act 2"),
    (dict(variant=3), "variant 3"),
    (dict(pitch=39), "pitch = 39 < t = 40"),
    (dict(k=0), "k = 0"),
]


def check_nc_refusal(pkg, r):
    over, cause = r
    kw = dict(cin=192, cout=192, k=3, t=40, batch=1)
    kw.update(over)
    with pytest.raises(pkg.VitsError) as e:
        pkg.op_norm_conv_plan(kw.pop("cin"), kw.pop("cout"), kw.pop("k"), kw.pop("t"), **kw)
    assert "vits_op_norm_conv" in str(e.value) and cause in str(e.value), str(e.value)


@pytest.mark.parametrize("r", NC_REFUSALS, ids=lambda r: "-".join("%s%d" % kv for kv in sorted(r[0].items())))
def test_norm_conv_refusals_name_their_cause(pkg, r):
    check_nc_refusal(pkg, r)
