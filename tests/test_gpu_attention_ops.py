"""The text encoder's attention kernels at operator level (rel_attention_kernel<1024 | 256> and the four instantiations of rel_attention_mfma_kernel, through
vits_op_attention), on inputs no whole model produces: a model reaches the short-sequence variant only on grids above 128 blocks and rel_attention_kernel<256>
only above 512, always at head size 96 and window 4, with q_scale = head_dim^-0.5, rows of 16-byte aligned pitch, and nothing but zeros behind lens[b].

Every variant is forced (vits_op_attention_plan says which instantiation runs and how many waves it has; the lengths are derived from those, lengths_of). The
batch is 4 utterances x 2 heads, lens = [T, T - 1, T - 2, T - 3] clipped at 1. Data: tests/attention_ref.py (unit-variance draws; a "peaked" draw with q and k x 4,
where one key dominates a row).

What is asserted:
  * the plan query names the kernel that was asked for;
  * bit identity, no tolerance: variants 3-6 (matrix cores) give the same bits as each other and variants 1-2 (VALU) as each other, on every valid column, at every
    head size x window x length, for both draws, with and without ggml's exponential table, q_scale 1 and head_dim^-0.5, and rows of pitch t rounded up to 4 (the
    16-byte V loads), that + 1 (the scalar V loads) and t + 67: the pitch changes no bit either;
  * the float64 anchor (q_scale = head_dim^-0.5, expf): per kernel family, rms error against float64 <= 2 x that of the sequential fp32 restatement, both relative
    to the reference's RMS (the 2x rule of tests/split_ref.py) — per length and draw where a case has 2000 outputs, and pooled over every length and both draws on
    the edge windows (queries within `window` of either end, the last query tile) and on the utterances whose last group of 16 keys is partial.
    Observed on an MI355X (the tests print every figure): restatement error 2.3e-8 to 1.9e-6 of RMS; GPU / restatement where asserted 0.81 to 1.07 (matrix cores)
    and 0.80 to 1.03 (VALU), worst at T = 15 ... 17; 0.88 to 1.14 on the cases below 2000 outputs (printed only); pooled 0.99 to 1.00 on the edge windows and on the
    utterances with a partial last key group, every head size and window;
  * with the table, the fp16 lookup decides: an fp32 score within rounding of an fp16 boundary takes the neighbouring entry, and such flips, not the accumulation
    order, are the whole difference to float64 (the restatement itself sits at 5e-8 ... 2e-5 of RMS, flips and all). There the bound is the format's: rms error
    <= 2^-11 of RMS (4.9e-4), half an fp16 unit, where flips at the restatement's rate cost 2e-5. Observed: 2.3e-8 to 3.7e-5 of RMS;
  * hygiene at T = 16 NW + 5: results finite, nothing but the staged 0xFF bytes behind lens[b], a lens = 0 row untouched and its neighbours unchanged, every row
    == its batch-1 call, the old vits_op_rel_attention == variant 0.
tests/test_encoder_op_host.py checks this file's case table and lengths on the CPU.
"""
import numpy as np
import pytest

import attention_ref as AR
import split_ref as R

pytestmark = pytest.mark.gpu
HEADS, BATCH = 2, 4
VALU, MFMA = (1, 2), (3, 4, 5, 6)
KERNEL = {1: "rel_attention_kernel<1024>", 2: "rel_attention_kernel<256>", 3: "rel_attention_mfma_kernel<4, 32, false, false>",
          4: "rel_attention_mfma_kernel<8, 32, false, false>", 5: "rel_attention_mfma_kernel<4, 24, true, false>", 6: "rel_attention_mfma_kernel<8, 24, false, true>"}
HEAD_DIMS = (16, 48, 80, 96, 128)  # ndt = 1, 3, 5, 6, 8 d tiles against 4 and 8 waves
VALU_HEAD_DIMS = (24, 40)          # no multiple of 16: the VALU kernels alone
WINDOWS = (0, 4, 8, 33)            # nrel = 1, 9, 17, 67: one tile of relative positions, past 16, past 16 NW
CASES = [(hd, w) for hd in HEAD_DIMS + VALU_HEAD_DIMS for w in WINDOWS]
NAN_BITS = 0xFFFFFFFF
TABLE_BOUND = 2.0 ** -11


def variants_of(hd):
    """the variants with an instantiation for this head size (the 24-step kernels stop at 96)"""
    if hd % 16:
        return VALU
    return VALU + tuple(v for v in MFMA if v <= 4 or hd <= 96)


def lengths_of(nws):
    """around one key tile, one and two rounds of the waves' key tiles, the V prefetch of the latency variant (128 keys), and past every one of them"""
    out = {1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 261}
    for nw in nws:
        out |= {16 * nw + 1, 32 * nw + 3}
    return sorted(out)


LENGTHS = tuple(lengths_of((4, 8)))  # every family runs every length: bit identity needs them in common


def ragged(T):
    return [max(1, T - i) for i in range(BATCH)]


def strides_of(T):
    a = (T + 3) // 4 * 4
    return (a, a + 1, T + 67)


def case_id(c):
    return "hd%d-w%d" % c


_TAB = []


def table():
    if not _TAB:
        _TAB.append(AR.exp_table())
    return _TAB[0]


def inputs(hd, w, T, peaked):
    return AR.make_case(HEADS, hd, w, T, BATCH, peaked)


def asserted_lengths(hd):
    """the lengths at which a case has MIN_OUTPUTS outputs, i.e. where the per-length rule is asserted and not only printed"""
    return [T for T in LENGTHS if HEADS * hd * sum(ragged(T)) >= AR.MIN_OUTPUTS]


def widen(x, ts, fill=7.5):
    """[B, C, T] -> [B, C, ts], garbage behind T"""
    return np.concatenate([x, np.full(x.shape[:2] + (ts - x.shape[2],), fill, np.float32)], axis=2) if ts > x.shape[2] else x


def run(pkg, data, w, T, lens, variant, q_scale=1.0, tab=None, ts=None):
    q, k, v, ek, ev = data
    ts = T if ts is None else ts
    out = pkg.op_attention(widen(q, ts), widen(k, ts), widen(v, ts), ek, ev, HEADS, w, q_scale=q_scale, variant=variant, exp_tab=tab, lens=lens, t=T)
    return out


def check_result(label, out, lens):
    """valid columns finite, every other element the staged 0xFF bytes"""
    for b, n in enumerate(lens):
        assert np.isfinite(out[b, :, :n]).all(), (label, b, "a value from behind lens[b] (NaN) was read")
        assert (out[b, :, n:].view(np.uint32) == NAN_BITS).all(), (label, b, "a column past lens[b] was written")
    return out


def same_bits(label, got, want, lens):
    for b, n in enumerate(lens):
        if not np.array_equal(got[b, :, :n], want[b, :, :n]):
            bad = np.argwhere(got[b, :, :n] != want[b, :, :n])
            raise AssertionError((label, "row", b, "len", n, "%d values differ; channels %d..%d, columns %d..%d" % (
                len(bad), bad[:, 0].min(), bad[:, 0].max(), bad[:, 1].min(), bad[:, 1].max()), float(np.abs(got[b, :, :n] - want[b, :, :n]).max())))


def plans(pkg, hd, w, T=1):
    out = {}
    for v in variants_of(hd):
        p = pkg.op_attention_plan(HEADS, hd, T, batch=BATCH, window=w, variant=v)
        assert p["variant"] == v and p["kernel"] == KERNEL[v], p
        out[v] = p
    return out


def combos(hd, T):
    """(q_scale, table, pitch): every value of each with every variant at every length and draw, not their full cross"""
    s0, s1, s2 = strides_of(T)
    qs = float(hd) ** -0.5
    return ((1.0, False, s0), (qs, True, s1), (qs, False, s2), (1.0, True, s0))


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_every_variant_of_a_family_gives_the_same_bits(pkg, c):
    hd, w = c
    pl = plans(pkg, hd, w)
    assert set(lengths_of({p["nw"] for p in pl.values() if p["nw"]} or {4, 8})) <= set(LENGTHS)
    families = [f for f in (VALU, tuple(v for v in MFMA if v in pl)) if f]
    for T in LENGTHS:
        lens = ragged(T)
        for peaked in (False, True):
            data = inputs(hd, w, T, peaked)
            for q_scale, tab, ts in combos(hd, T):
                for fam in families:
                    want = None
                    for v in fam:
                        label = "%s variant %d T %d peaked %d q_scale %.3g table %d pitch %d" % (case_id(c), v, T, peaked, q_scale, tab, ts)
                        got = check_result(label, run(pkg, data, w, T, lens, v, q_scale, table() if tab else None, ts), lens)
                        if want is None:
                            want = got
                        else:
                            same_bits(label + " vs variant %d" % fam[0], got, want, lens)
            for fam in families:  # the pitch changes no bit: same q_scale, no table, the three pitches, one variant per family
                s0, s1, s2 = strides_of(T)
                a = run(pkg, data, w, T, lens, fam[-1], 1.0, None, s0)
                for ts in (s1, s2):
                    same_bits("%s variant %d T %d pitch %d vs %d" % (case_id(c), fam[-1], T, ts, s0), run(pkg, data, w, T, lens, fam[-1], 1.0, None, ts), a, lens)


class Pool:
    """squared errors of the GPU result and of the restatement on a set of outputs, pooled over calls: the 2x rule on them alone"""

    def __init__(self):
        self.g = self.rg = self.c = self.rc = 0.0
        self.n = 0

    def add(self, cols, ref, chain, rows, mask):
        if not mask.any():
            return
        r = ref[:, mask]
        self.g += float(((cols[:, mask].astype(np.float64) - r) ** 2).sum())
        self.rg += float((r ** 2).sum())
        self.c += float(((chain[:, mask].astype(np.float64) - r[rows]) ** 2).sum())
        self.rc += float((r[rows] ** 2).sum())
        self.n += int(mask.sum()) * r.shape[0]

    def ratio(self):
        return np.sqrt(self.g / self.rg) / (np.sqrt(self.c / self.rc) + 1e-300)


def anchor_families(hd):
    """one variant per family (the identity test ties the others to it): the long four-wave kernel and the sixteen-wave VALU kernel"""
    return ((3, "mfma"), (1, "valu")) if hd % 16 == 0 else ((1, "valu"),)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_each_family_against_float64(pkg, c):
    hd, w = c
    q_scale = float(hd) ** -0.5
    rows = np.arange(HEADS * hd)  # (the restatement runs on every output: the ratio compares like with like)
    fams = anchor_families(hd)
    edge = {name: Pool() for _, name in fams}
    part = {name: Pool() for _, name in fams}
    asserted = 0
    for T in LENGTHS:
        lens = ragged(T)
        m_edge, m_part = AR.edge_queries(lens, w), AR.partial_group_queries(lens)
        for peaked in (False, True):
            q, k, v, ek, ev = data = inputs(hd, w, T, peaked)
            ref = R.gather_cols(AR.reference64(q, k, v, ek, ev, HEADS, w, lens, q_scale), lens)
            chain = R.gather_cols(AR.chain32(q, k, v, ek, ev, HEADS, w, lens, q_scale), lens)
            c_rms, c_max = R.rms_err(chain, ref[rows])
            ref_t = R.gather_cols(AR.reference64(q, k, v, ek, ev, HEADS, w, lens, q_scale, table()), lens)
            for variant, name in fams:
                label = "%s %s T %d peaked %d" % (case_id(c), name, T, peaked)
                cols = R.gather_cols(check_result(label, run(pkg, data, w, T, lens, variant, q_scale), lens), lens)
                g_rms, g_max = R.rms_err(cols, ref)
                t_rms, _ = R.rms_err(R.gather_cols(check_result(label + " table", run(pkg, data, w, T, lens, variant, q_scale, table()), lens), lens), ref_t)
                print("%s: %d outputs: gpu rms %.2e max %.2e of RMS; restatement rms %.2e max %.2e; ratio %.2f; with the table %.2e of RMS" % (
                    label, cols.size, g_rms, g_max, c_rms, c_max, g_rms / c_rms, t_rms))
                edge[name].add(cols, ref, chain, rows, m_edge)
                part[name].add(cols, ref, chain, rows, m_part)
                assert t_rms <= TABLE_BOUND, (label, "table", t_rms)
                if cols.size >= AR.MIN_OUTPUTS:
                    assert g_rms <= AR.FACTOR * c_rms, (label, g_rms, c_rms)
                    asserted += 1
    assert asserted == len(fams) * 2 * len(asserted_lengths(hd)) and len(asserted_lengths(hd)) >= 9, asserted  # (T = 1, 2; at head size 16 also 15, 16, 17 are printed only)
    for _, name in fams:
        print("%s %s pooled over every length and both draws: edge windows %.2f (%d outputs), partial last key group %.2f (%d outputs)" % (
            case_id(c), name, edge[name].ratio(), edge[name].n, part[name].ratio(), part[name].n))
        assert edge[name].n >= AR.MIN_OUTPUTS and edge[name].ratio() <= AR.FACTOR, (name, "edge windows", edge[name].ratio())
        assert part[name].n >= AR.MIN_OUTPUTS and part[name].ratio() <= AR.FACTOR, (name, "partial last key group", part[name].ratio())


HYGIENE = [(96, 4, v) for v in VALU + MFMA] + [(128, 33, 4), (24, 8, 1), (24, 8, 2)]


@pytest.mark.parametrize("h", HYGIENE, ids=lambda h: "hd%d-w%d-v%d" % h)
def test_rows_strides_and_empty_rows(pkg, h):
    hd, w, variant = h
    nw = pkg.op_attention_plan(HEADS, hd, 1, batch=BATCH, window=w, variant=variant)["nw"] or 8
    T = 16 * nw + 5
    lens = ragged(T)
    data = AR.make_case(HEADS, hd, w, T, BATCH, False)
    q_scale = float(hd) ** -0.5
    plain = check_result("plain", run(pkg, data, w, T, lens, variant, q_scale), lens)
    # every row == its batch-1 call
    for b, n in enumerate(lens):
        alone = pkg.op_attention(*(x[b:b + 1, :, :n] for x in data[:3]), data[3], data[4], HEADS, w, q_scale=q_scale, variant=variant, lens=[n])
        assert np.array_equal(alone[0], plain[b, :, :n]), ("a row of the ragged batch != its batch-1 call", b)
    # a row with lens = 0 comes back as staged, its neighbours with the same bits
    lens0 = [T, 0, T - 2, T - 3]
    got0 = check_result("lens 0", run(pkg, data, w, T, lens0, variant, q_scale), lens0)
    assert (got0[1].view(np.uint32) == NAN_BITS).all(), "a row with lens = 0 was written"
    for b in (0, 2, 3):
        assert np.array_equal(got0[b, :, :lens0[b]], plain[b, :, :lens0[b]]), ("a row next to an empty row changed", b)
    # no lens at all: every row runs to t
    full = run(pkg, data, w, T, None, variant, q_scale)
    assert np.isfinite(full).all() and np.array_equal(full[0], plain[0])


@pytest.mark.parametrize("c", [(96, 4), (24, 4), (128, 8)], ids=case_id)
def test_the_old_entry_point_gives_the_bits_of_variant_0(pkg, c):
    hd, w = c
    T = 16 * 8 + 5
    lens = ragged(T)
    q, k, v, ek, ev = data = AR.make_case(HEADS, hd, w, T, BATCH, False)
    old = pkg.op_rel_attention(q, k, v, ek, ev, HEADS, w, lens=lens)
    plan = pkg.op_attention_plan(HEADS, hd, T, batch=BATCH, window=w)
    assert plan["variant"] in variants_of(hd)
    new = check_result("variant 0", run(pkg, data, w, T, lens, 0), lens)
    same_bits("vits_op_rel_attention vs vits_op_attention variant 0", old, new, lens)
    same_bits("variant 0 vs the variant it names", run(pkg, data, w, T, lens, plan["variant"]), new, lens)


REFUSALS = [
    # (head_dim, window, t, variant, what the message names)
    (144, 4, 40, 0, "head_dim = 144"),
    (144, 4, 40, 1, "head_dim = 144"),
    (24, 4, 40, 3, "head_dim = 24 is not a multiple of 16"),
    (40, 4, 40, 6, "head_dim = 40 is not a multiple of 16"),
    (128, 4, 40, 5, "head_dim = 128 is above 96"),
    (112, 4, 40, 6, "head_dim = 112 is above 96"),
    (96, 4, 2600, 3, "bytes of LDS, the limit is 163840"),
    (96, 4, 2600, 6, "bytes of LDS, the limit is 163840"),
    (96, 4, 2400, 1, "bytes of LDS, the limit is 153600"),
    (96, 4, 40, 7, "variant 7"),
    (96, -1, 40, 0, "window = -1"),
]


def refusal_id(r):
    return "hd%d-w%d-t%d-v%d" % r[:4]


def check_refusal(pkg, r):
    hd, w, T, variant, cause = r
    with pytest.raises(pkg.VitsError) as e:
        pkg.op_attention_plan(HEADS, hd, T, batch=2, window=w, variant=variant)
    assert "vits_op_attention" in str(e.value) and cause in str(e.value), str(e.value)
    # the op itself: the same message, before any device call (this runs on a machine without a GPU as well)
    z = np.zeros((2, HEADS * hd, T), np.float32)
    rel = np.zeros((2 * max(w, 0) + 1, hd), np.float32)
    d = pkg.AttentionDesc(2, HEADS, hd, T, T, w, 1.0, variant)
    import ctypes as C
    out = np.zeros_like(z)
    assert pkg.lib().vits_op_attention(C.byref(d), pkg._ptr(z), pkg._ptr(z), pkg._ptr(z), pkg._ptr(rel), pkg._ptr(rel), None, None, pkg._ptr(out)) != 0
    assert pkg.last_error() == str(e.value)


@pytest.mark.parametrize("r", REFUSALS, ids=refusal_id)
def test_refusals_name_their_cause_and_never_fall_back(pkg, r):
    check_refusal(pkg, r)
