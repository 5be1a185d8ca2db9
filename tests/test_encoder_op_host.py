"""vits_op_attention, vits_op_layer_norm and vits_op_norm_conv without a GPU: the plan queries (host arithmetic only) over the case tables of
tests/test_gpu_attention_ops.py and tests/test_gpu_norm_ops.py — imported, not restated — prove that every case names the kernel it means, that forcing does not
depend on the grid, that the forced plans are the launch-plan tables' (name, grid, block, LDS bytes), that every attention and LayerNorm instantiation those tables
list is run by an operator test, and that no case table is silently empty; the refusals come back before any device call; the ctypes structs follow the header;
and the numpy references agree with each other where they must."""
import os
import re

import numpy as np
import pytest

import attention_ref as AR
import norm_ref as NR
import split_ref as R
import test_gpu_attention_ops as GA
import test_gpu_norm_ops as GN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_plan_table.txt")
HEADER = os.path.join(ROOT, "include", "vits.h")


def golden_rows(family):
    """(case ints, kernel, (gx, gy, gz, block, lds)) of the default knob set's launchable rows of one family of the golden launch-plan table"""
    out, default = [], False
    for line in open(GOLDEN).read().splitlines():
        if line.startswith("## "):
            default = line[3:] == "default"
        elif default and line.startswith(family + " "):
            key, fields = line.split(" : ", 1)
            m = re.search(r"(\w+_kernel<[^>]*>) \| (\d+) (\d+) (\d+) (\d+) (\d+)", fields)
            if m:
                out.append(([int(v) for v in key.split()[1:]], m.group(1), tuple(int(v) for v in m.groups()[1:])))
    return out


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------------------------
def header_fields(struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), open(HEADER).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*\]", "", n).strip() for n in decl.split(None, 1)[1].split(",")]
    return names


@pytest.mark.parametrize("struct, cls", [("vits_attention_desc", "AttentionDesc"), ("vits_attention_plan", "AttentionPlan"), ("vits_layer_norm_desc", "LayerNormDesc"),
                                         ("vits_layer_norm_plan", "LayerNormPlan"), ("vits_norm_conv_desc", "NormConvDesc"), ("vits_norm_conv_plan", "NormConvPlan")])
def test_the_ctypes_structs_follow_the_header(pkg, struct, cls):
    assert [n for n, _ in getattr(pkg, cls)._fields_] == header_fields(struct)


def test_the_entry_points_are_declared_exported_and_wrapped(pkg):
    header = open(HEADER).read()
    for name in ("vits_op_attention", "vits_op_layer_norm", "vits_op_norm_conv"):
        for sym in (name, name + "_plan"):
            assert "VITS_API int %s(" % sym in header and sym in pkg.EXPORTED_SYMBOLS and hasattr(pkg.lib(), sym), sym
        assert callable(getattr(pkg, name[5:])) and callable(getattr(pkg, name[5:] + "_plan"))
    # the argument counts of the declarations are the wrappers'
    for sym, n in (("vits_op_attention", 9), ("vits_op_layer_norm", 8), ("vits_op_norm_conv", 10)):
        decl = re.search(r"VITS_API int %s\((.*?)\);" % sym, header, re.S).group(1)
        assert len(decl.split(",")) == n == len(getattr(pkg.lib(), sym).argtypes), sym


# ---- attention --------------------------------------------------------------------------------------------------------------------------------------------------
def test_attention_cases_lengths_and_counts():
    assert len(GA.CASES) == 28 and len(set(GA.CASES)) == 28
    assert GA.LENGTHS == (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 131, 259, 261)
    assert set(GA.lengths_of((4,))) | set(GA.lengths_of((8,))) == set(GA.LENGTHS)
    assert {hd // 16 for hd in GA.HEAD_DIMS} == {1, 3, 5, 6, 8} and {2 * w + 1 for w in GA.WINDOWS} == {1, 9, 17, 67}
    for T in (4, 17, 261):
        assert sorted(n % 4 for n in GA.ragged(T)) == [0, 1, 2, 3]
    assert GA.ragged(1) == [1, 1, 1, 1]
    for T in GA.LENGTHS:  # an aligned pitch, one that is no multiple of 4, a far larger one
        a, b, c = GA.strides_of(T)
        assert a % 4 == 0 and a >= T and b == a + 1 and c >= T + 64
    # every (variant, head size) with an instantiation is run; the per-length rule is asserted at nine lengths or more per family and head size
    ran = {(v, hd) for hd, _ in GA.CASES for v in GA.variants_of(hd)}
    assert ran == {(v, hd) for hd in GA.HEAD_DIMS + GA.VALU_HEAD_DIMS for v in (1, 2)} | {(v, hd) for hd in GA.HEAD_DIMS for v in (3, 4)} | {
        (v, hd) for hd in GA.HEAD_DIMS if hd <= 96 for v in (5, 6)}
    for hd in GA.HEAD_DIMS + GA.VALU_HEAD_DIMS:
        assert len(GA.asserted_lengths(hd)) >= 9 and GA.anchor_families(hd)[-1] == (1, "valu") and (hd % 16 != 0 or GA.anchor_families(hd)[0] == (3, "mfma"))
    assert {c[0] for c in GA.combos(96, 17)} == {1.0, 96.0 ** -0.5}
    assert {c[1] for c in GA.combos(96, 17)} == {False, True} and {c[2] for c in GA.combos(96, 17)} == set(GA.strides_of(17))
    # the edge windows and the partial-group utterances are what they say
    lens = [20, 16, 3]
    e = AR.edge_queries(lens, 2)
    assert e.sum() == (2 + 4) + 16 + 3 and e.size == 39  # (the window at the head + the last query tile, which holds the window at the tail; one tile: all of it)
    assert AR.partial_group_queries(lens).tolist() == [True] * 20 + [False] * 16 + [True] * 3


@pytest.mark.parametrize("c", GA.CASES, ids=GA.case_id)
def test_every_attention_case_names_its_kernel_whatever_the_grid(pkg, c):
    hd, w = c
    for T, B in ((1, 1), (131, 4), (513, 64), (2049, 1)):
        for v in GA.variants_of(hd):
            try:
                p = pkg.op_attention_plan(GA.HEADS, hd, T, batch=B, window=w, variant=v)
            except pkg.VitsError as e:
                assert T == 2049 and "bytes of LDS" in str(e), (v, T, str(e))  # (only the LDS limit depends on the length)
                continue
            assert p["kernel"] == GA.KERNEL[v] and p["variant"] == v and p["grid"] == ((T + 15) // 16, GA.HEADS, B), p
            assert (p["nw"], p["maxs"]) == {1: (0, 0), 2: (0, 0), 3: (4, 32), 4: (8, 32), 5: (4, 24), 6: (8, 24)}[v] and p["block"] == (64 * p["nw"] or (1024, 256)[v - 1])
    nws = {pkg.op_attention_plan(GA.HEADS, hd, 1, batch=4, window=w, variant=v)["nw"] for v in GA.variants_of(hd)} - {0}
    assert set(GA.lengths_of(nws or {4, 8})) <= set(GA.LENGTHS)


def test_forced_attention_plans_are_the_launch_plan_tables(pkg):
    """Every launchable AT row of the golden table (default knobs), asked for by variant: the same name, grid, block and LDS bytes; variant 0 picks the row's kernel;
    and every instantiation the table lists is one an operator test runs."""
    variant_of = {k: v for v, k in GA.KERNEL.items()}
    rows = golden_rows("AT")
    assert len(rows) > 100
    seen = set()
    for (heads, hd, w, T, B), kernel, (gx, gy, gz, block, lds) in rows:
        for variant in (variant_of[kernel], 0):
            p = pkg.op_attention_plan(heads, hd, T, batch=B, window=w, variant=variant)
            assert (p["kernel"], p["grid"], p["block"], p["lds"]) == (kernel, (gx, gy, gz), block, lds), ((heads, hd, w, T, B), variant, p)
        seen.add(kernel)
    assert seen == set(GA.KERNEL.values())
    assert {GA.KERNEL[v] for hd, _ in GA.CASES for v in GA.variants_of(hd)} == seen, "an attention instantiation of the tables that no operator test runs"


@pytest.mark.parametrize("r", GA.REFUSALS, ids=GA.refusal_id)
def test_attention_refusals_come_back_without_a_gpu(pkg, r):
    GA.check_refusal(pkg, r)


def test_bad_lens_are_refused_before_any_device_call(pkg):
    q = np.zeros((2, 32, 8), np.float32)
    rel = np.zeros((9, 16), np.float32)
    x = np.zeros((2, 16, 8), np.float32)
    g = np.ones(16, np.float32)
    w = np.zeros((32, 16, 3), np.float32)
    for lens in ([9, 1], [-1, 1]):
        for call in (lambda: pkg.op_attention(q, q, q, rel, rel, 2, 4, variant=1, lens=lens), lambda: pkg.op_layer_norm(x, g, g, lens=lens),
                     lambda: pkg.op_norm_conv(x, g, g, w, variant=1, lens=lens)):
            with pytest.raises(pkg.VitsError) as e:
                call()
            assert "lens[b] <= t" in str(e.value), str(e.value)


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------------------------------------------
def test_layer_norm_cases_plans_and_refusals(pkg):
    assert len(GN.LN_CASES) == 30 and GN.LN_LENGTHS == (1, 2, 31, 32, 33, 63, 64, 65, 67, 131)
    assert {C % 16 for C in GN.CHANNELS} >= {0, 5, 8, 13} and any(C < 16 for C in GN.CHANNELS) and any(C > 192 for C in GN.CHANNELS)  # the load loop's tails
    for C in GN.CHANNELS:
        assert len(GN.asserted_ln_lengths(C)) >= 1, C
        for tw in GN.TWS:
            for T, B in ((1, 1), (131, 4), (100000, 64)):
                p = pkg.op_layer_norm_plan(C, T, batch=B, tw=tw)
                assert p == dict(kernel="add_layer_norm_kernel<%d>" % tw, tw=tw, grid=((T + tw - 1) // tw, B, 1), block=16 * tw, lds=4 * (C * tw + 32 * tw)), p
        assert pkg.op_layer_norm_plan(C, 40)["tw"] == 32
    # the tables' rows: the tile of 32 under the default knobs, the tile of 64 under ln_tw=64, same grid, block and LDS bytes
    table = open(GOLDEN).read()
    for tw, knobs in ((32, "default"), (64, "ln_tw=64")):
        section = table.split("## %s\n" % knobs)[1].split("## ")[0]
        rows = re.findall(r"^LN (\d+) (\d+) (\d+) : 1 (add_layer_norm_kernel<\d+>) \| (\d+) (\d+) (\d+) (\d+) (\d+)", section, re.M)
        assert len(rows) >= 6
        for C, T, B, kernel, gx, gy, gz, block, lds in rows:
            p = pkg.op_layer_norm_plan(int(C), int(T), batch=int(B), tw=tw)
            assert (p["kernel"], p["grid"], p["block"], p["lds"]) == (kernel, (int(gx), int(gy), int(gz)), int(block), int(lds)), (C, T, B, p)
    for kw, cause in ((dict(tw=48), "tw = 48"), (dict(tw=64, channels=569), "bytes of LDS for channels = 569"), (dict(tw=32, channels=1169), "bytes of LDS for channels = 1169")):
        with pytest.raises(pkg.VitsError) as e:
            pkg.op_layer_norm_plan(kw.get("channels", 192), 40, tw=kw["tw"])
        assert "vits_op_layer_norm" in str(e.value) and cause in str(e.value), str(e.value)
    x, g = np.zeros((1, 16, 8), np.float32), np.ones(16, np.float32)
    with pytest.raises(pkg.VitsError) as e:
        pkg.op_layer_norm(x, g, g, gelu_tab=NR.gelu_table())
    assert "gelu_tab without post_gelu" in str(e.value)


# ---- LayerNorm on load ------------------------------------------------------------------------------------------------------------------------------------------
def test_norm_conv_cases_and_plans(pkg):
    assert len(GN.NC_CASES) == 36 and GN.NC_LENGTHS == (1, 2, 15, 16, 17, 31, 33, 40)
    assert [GN.pads_of(k) for k in GN.NC_K] == [[0], [0, 1, 2], [0, 2, 4]]
    n2 = 0
    for cin, cout, k in GN.NC_CASES:
        for pad in GN.pads_of(k):
            for T in GN.NC_LENGTHS:
                for B in (1, GN.BATCH):
                    p = pkg.op_norm_conv_plan(cin, cout, k, T, batch=B, pad_left=pad)
                    assert p["tile"] == "TILE_LAT16" and p["pitch"] == (T + 31) // 32 * 32 and p["grid"] == ((T + 15) // 16, (cout + 63) // 64, B), p
                    assert p["ln_ok"] == (cin <= GN.LN_ON_LOAD_MAX_CIN) and p["variant"] == (2 if p["ln_ok"] else 1) and p["launches"] == 3 - p["variant"], p
                    assert (p["ln_why"] == "") == p["ln_ok"]
                    n2 += p["ln_ok"]
    assert n2 == 9 * 7 * 8 * 2  # (the nine (cin, cout) with cin <= 768 normalise on load: 7 paddings over the three kernel sizes, 8 lengths, 2 batches)
    assert {(cout + 63) // 64 for cout in GN.NC_COUT} == {1, 3, 9}
    # the statistics' scratch beside the input tile: 4 KB of partial sums + gamma and beta
    a, b = pkg.op_norm_conv_plan(192, 192, 3, 40, variant=1), pkg.op_norm_conv_plan(192, 192, 3, 40, variant=2)
    assert b["lds"] - a["lds"] == 4 * (2 * 16 * 32 + 2 * 192)
    assert pkg.op_norm_conv_plan(192, 192, 3, 33, pitch=37)["pitch"] == 37
    assert all(GN.odd_pitch(T) % 4 and GN.odd_pitch(T) >= T for T in GN.NC_LENGTHS) and GN.odd_pitch(33) == 37


@pytest.mark.parametrize("r", GN.NC_REFUSALS, ids=lambda r: "-".join("%s%d" % kv for kv in sorted(r[0].items())))
def test_norm_conv_refusals_come_back_without_a_gpu(pkg, r):
    GN.check_nc_refusal(pkg, r)


# ---- the references against each other --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd, w, T", [(16, 0, 17), (48, 4, 40), (96, 33, 67)])
def test_attention_references(hd, w, T):
    lens = GA.ragged(T)
    rows = np.arange(hd)
    tab = AR.exp_table()
    for peaked in (False, True):
        q, k, v, ek, ev = AR.make_case(GA.HEADS, hd, w, T, GA.BATCH, peaked)
        qs = float(hd) ** -0.5
        ref = AR.reference64(q, k, v, ek, ev, GA.HEADS, w, lens, qs)
        chain = AR.chain32(q[:, :hd], k[:, :hd], v[:, :hd], ek, ev, 1, w, lens, qs)
        for b, n in enumerate(lens):
            assert not ref[b, :, n:].any() and not chain[b, :, n:].any()
        # the closed form, term by term, on one query
        b, h, i = 1, 1, min(3, lens[1] - 1)
        n = lens[b]
        qi = (q[b, h * hd:(h + 1) * hd, i] * np.float32(qs)).astype(np.float64)
        s = np.array([qi @ k[b, h * hd:(h + 1) * hd, j].astype(np.float64) + (qi @ ek[j - i + w].astype(np.float64) if abs(j - i) <= w else 0.0) for j in range(n)])
        p = np.exp(s - s.max()) / np.exp(s - s.max()).sum()
        o = sum(p[j] * (v[b, h * hd:(h + 1) * hd, j].astype(np.float64) + (ev[j - i + w] if abs(j - i) <= w else 0.0)) for j in range(n))
        assert np.allclose(ref[b, h * hd:(h + 1) * hd, i], o, rtol=1e-12, atol=1e-12)
        # the restatement: fp32 accuracy, and a denominator of the rule that is not zero
        c_rms, c_max = R.rms_err(R.gather_cols(chain, lens), R.gather_cols(ref, lens)[rows])
        assert 1e-8 < c_rms < 1e-5, c_rms
        # the table path against a direct fp16 evaluation: exp of the fp16-rounded argument, rounded to fp16
        x = np.linspace(-12, 0, 4001).astype(np.float32)
        direct = np.exp(x.astype(np.float16).astype(np.float64)).astype(np.float16).astype(np.float32)
        assert np.array_equal(AR.table_lookup(tab, x), direct)
        ref_t = AR.reference64(q, k, v, ek, ev, GA.HEADS, w, lens, qs, tab)
        chain_t = AR.chain32(q[:, :hd], k[:, :hd], v[:, :hd], ek, ev, 1, w, lens, qs, tab)
        t_rms, _ = R.rms_err(R.gather_cols(chain_t, lens), R.gather_cols(ref_t, lens)[rows])
        d_rms, _ = R.rms_err(R.gather_cols(ref_t, lens), R.gather_cols(ref, lens))
        print("hd %d w %d T %d peaked %d: restatement %.2e of RMS; with the table %.2e; the table against expf %.2e" % (hd, w, T, peaked, c_rms, t_rms, d_rms))
        assert t_rms < GA.TABLE_BOUND / 4 and 1e-6 < d_rms < 4 * GA.TABLE_BOUND, (t_rms, d_rms)


@pytest.mark.parametrize("hd, w, T, peaked", [(96, 4, 131, False), (96, 4, 131, True), (48, 33, 65, True)])
def test_the_rule_catches_what_an_attention_kernel_could_get_wrong(hd, w, T, peaked):
    """Seeded faults against the 2x rule, each far beyond it: the relative-key and the relative-value columns shifted by one position, and the last key of a partial
    group of 16 dropped from P V. Measured 5e4 to 2e6 x the restatement."""
    lens = GA.ragged(T)
    q, k, v, ek, ev = AR.make_case(GA.HEADS, hd, w, T, GA.BATCH, peaked)
    qs = float(hd) ** -0.5
    ref = R.gather_cols(AR.reference64(q, k, v, ek, ev, GA.HEADS, w, lens, qs), lens)
    c_rms, _ = R.rms_err(R.gather_cols(AR.chain32(q, k, v, ek, ev, GA.HEADS, w, lens, qs), lens), ref)
    dropped = v.copy()
    for b, n in enumerate(lens):
        if n % 16:
            dropped[b, :, n - 1] = 0
    faults = {"rel_k shifted": (q, k, v, np.roll(ek, 1, axis=0), ev), "rel_v shifted": (q, k, v, ek, np.roll(ev, 1, axis=0)), "last key dropped": (q, k, dropped, ek, ev)}
    part = AR.partial_group_queries(lens)
    for name, data in faults.items():
        got = R.gather_cols(AR.reference64(*data, GA.HEADS, w, lens, qs), lens).astype(np.float32)
        g_rms, _ = R.rms_err(got, ref)
        p_rms, _ = R.rms_err(got[:, part], ref[:, part])
        print("%s: %.3g x the restatement overall, %.3g x on the utterances with a partial last key group" % (name, g_rms / c_rms, p_rms / c_rms))
        assert g_rms > 1000 * AR.FACTOR * c_rms and p_rms > 1000 * AR.FACTOR * c_rms, (name, g_rms, c_rms)


@pytest.mark.parametrize("C, T", [(5, 33), (29, 67), (200, 40)])
def test_layer_norm_references(C, T):
    lens = GN.ragged(T)
    tab = NR.gelu_table()
    for offset in (False, True):
        x, res, y0, gamma, beta = NR.make_case(C, T, GN.BATCH, offset)
        for kw in (dict(), dict(gelu=True)):
            ref, chain = NR.reference64(x, res, gamma, beta, 1e-5, lens, **kw), NR.chain32(x, res, gamma, beta, 1e-5, lens, **kw)
            c_rms, _ = R.rms_err(chain, ref)
            assert 1e-8 < c_rms < (1e-4 if offset else 2e-6), (C, T, offset, kw, c_rms)
        # a one-pass variance would not survive the offset draw: the two-pass restatement does
        v = (R.gather_cols(x, lens) + R.gather_cols(res, lens)).astype(np.float32)
        one_pass = ((v * v).astype(np.float32).mean(axis=0, dtype=np.float32) - v.mean(axis=0, dtype=np.float32) ** 2).astype(np.float32)
        two_pass = v.astype(np.float64).var(axis=0)
        if offset:
            assert np.abs(one_pass - two_pass).max() > 1e-4 * two_pass.max()
        # the first column by hand
        col = x[0, :, 0].astype(np.float64) + res[0, :, 0].astype(np.float64)
        want = (col - col.mean()) / np.sqrt(col.var() + np.float64(np.float32(1e-5))) * gamma + beta
        assert np.allclose(NR.reference64(x, res, gamma, beta, 1e-5, lens)[:, 0], want, rtol=1e-12, atol=1e-12)
        # the table path against a direct fp16 evaluation of ggml's tanh-GELU
        y = np.linspace(-6, 6, 4001).astype(np.float32)
        h = y.astype(np.float16).astype(np.float64)
        direct = (0.5 * h * (1 + np.tanh(np.sqrt(2 / np.pi) * h * (1 + 0.044715 * h * h)))).astype(np.float16).astype(np.float32)
        assert np.array_equal(NR.table_lookup(tab, y), direct)
        t_rms, _ = R.rms_err(NR.chain32(x, res, gamma, beta, 1e-5, lens, gelu_tab=tab), NR.reference64(x, res, gamma, beta, 1e-5, lens, gelu_tab=tab))
        assert t_rms < GN.TABLE_BOUND / 4, t_rms
    m = NR.edge_columns([70, 32, 1], 32)
    assert np.flatnonzero(m).tolist() == [31, 32, 63, 64, 69, 70 + 31, 70 + 32]
