"""The operator entries of the stochastic duration predictor without a GPU: tests/dp_ref.py's spline against the oracle's (vo_spline: spline_inverse and
unconstrained_spline_reference, the second opinion), the case tables of tests/test_gpu_dds_ops.py and tests/test_gpu_spline_ops.py — imported, not restated —
against the plan queries (host arithmetic only), the refusals, and the condition the exact durations test rests on."""
import os
import re

import numpy as np
import pytest

import dp_ref as D
import oracle_lib as O
import test_gpu_dds_ops as G
import test_gpu_spline_ops as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plan_table.txt")
INV_SQRT = S.INV_SQRT
# every instantiation the launchers can name (dds.hip VITS_DDS_LAUNCH, stage1_lat.hip VITS_DDSL_M)
LAYER_KERNELS = {"dds_layer_kernel<%d, %d>" % (a, m) for a in (0, 1, 2) for m in (2, 4, 6, 8)}
LAT_KERNELS = {"dds_layer_lat_kernel<%d, %d, %d>" % (h, t, m) for h in (0, 1, 2) for t in (0, 1) for m in (6, 8)}
assert O.MODE_REFERENCE == D.MODE_REFERENCE and O.MODE_HF == D.MODE_HF

PLACES = {"none": lambda n: [], "first": lambda n: [0], "last": lambda n: [n - 1], "all": lambda n: list(range(n)),
          "scattered": lambda n: [0, 5, 6, n // 2, n - 1]}


def spline_errors(bins, scale, mode, place, T=4000, seed=11):
    u, zr, tail = D.make_spline_case(T, bins, seed + bins, scale, PLACES[place](T))
    if place != "all":
        zr[2], zr[3] = np.float32(tail), -np.float32(tail)  # the bounds are inside
    ref = D.spline(zr, u, bins, tail, INV_SQRT, mode, np.float64)
    chain = D.spline(zr, u, bins, tail, INV_SQRT, mode, np.float32)
    orc = O.spline(u, zr, bins, tail, INV_SQRT, mode)
    return zr, u, tail, ref, chain, orc


@pytest.mark.parametrize("place", list(PLACES))
@pytest.mark.parametrize("mode", [D.MODE_HF, D.MODE_REFERENCE], ids=["hf", "reference"])
@pytest.mark.parametrize("c", S.SPLINE_CASES, ids=S.spline_id)
def test_spline_reference_agrees_with_the_oracle(c, mode, place):
    """float64 dp_ref.spline against the oracle's fp32 spline: within the float32 restatement's own error (the factors of the GPU test); the restatement's
    figures on 4000 tokens are printed (10 bins, unit: rms 7e-7, max 2e-5 of a result of RMS 2.9)"""
    bins, scale = c
    zr, u, tail, ref, chain, orc = spline_errors(bins, scale, mode, place)
    inside = np.abs(zr) <= np.float32(tail)
    if mode == D.MODE_HF:
        assert np.array_equal(orc[~inside].view(np.uint32), zr[~inside].view(np.uint32)) and np.array_equal(ref[~inside], zr[~inside].astype(np.float64))
    if not inside.any():
        assert np.array_equal(orc.astype(np.float64), ref)  # (reference mode: zeros, forwarded)
        return
    e_o, e_c = np.abs(orc[inside] - ref[inside]), np.abs(chain[inside] - ref[inside])
    rms = lambda e: float(np.sqrt((e ** 2).mean()))
    print("%s mode %d %s: RMS of the result %.2f; restatement rms %.2e max %.2e; oracle rms %.2e max %.2e"
          % (S.spline_id(c), mode, place, rms(ref[inside]), rms(e_c), e_c.max(), rms(e_o), e_o.max()))
    assert rms(e_o) <= S.RMS_FACTOR * rms(e_c) and e_o.max() <= S.MAX_FACTOR * e_c.max()


@pytest.mark.parametrize("place", list(PLACES))
@pytest.mark.parametrize("c", S.SPLINE_CASES, ids=S.spline_id)
def test_reference_mode_sources_are_the_oracles(c, place):
    """which token's result (or which masked input) every token receives: the oracle's output is nearest to the candidate dp_ref.spline_sources names"""
    bins, scale = c
    zr, u, tail, ref, chain, orc = spline_errors(bins, scale, D.MODE_REFERENCE, place, T=700)
    inside, src = D.spline_sources(zr, tail)
    n = zr.size
    vals = np.where(inside, zr, np.float32(0))
    told_apart = S.check_sources(orc, zr, u, bins, tail, place)
    assert np.array_equal(orc[~inside].view(np.uint32), vals[src[~inside]].view(np.uint32))
    assert told_apart > 0 or place in ("none", "all") or bins == 1
    if place == "scattered":  # the pair really shifts tokens: token 1 (inside, first inside token) holds the result of token 0, an outside one
        assert src[1] == 0 and not inside[0] and src[n - 2] < n - 2


def test_spline_refusals_need_no_gpu(pkg):
    S.check_spline_refusals(pkg)


# ---- the DDS case table against the plan query -----------------------------------------------------------------------------------------------------
def golden_names():
    with open(GOLDEN) as f:
        return set(re.findall(r"dds_layer(?:_lat)?_kernel<[^>]*>", f.read()))


def test_the_launch_plan_table_prints_names_of_the_same_form():
    names = golden_names()
    assert names and names <= LAYER_KERNELS | LAT_KERNELS, names - LAYER_KERNELS - LAT_KERNELS


@pytest.mark.parametrize("c", G.CASES + G.WIDE_CASES, ids=G.case_id)
def test_every_dds_case_names_its_kernels_and_its_lengths_hit_the_edges(pkg, c):
    pad = (c["k"] - 1) * c["k"] ** (c["layers"] - 1) // 2
    for variant, nt, arithes in ((G.LAYER, 32, (G.F32, G.F16, G.BF16)), (G.LAT, 16, (G.F32,))):
        for arith in arithes:
            ends = G.lat_ends(c) if variant == G.LAT and c in G.CASES else [(0, 0)]
            for head, tail in ends:
                if variant == G.LAT and c["layers"] > 3:
                    continue  # (refused: REFUSALS)
                plan = G.plan_of(pkg, c, variant, arith, 1, head, tail)
                first, last = G.expected_kernels(c, variant, arith, head, tail)
                assert (plan["kernel"], plan["kernel_last"]) == (first, last) and {first, last} <= LAYER_KERNELS | LAT_KERNELS
                assert plan["variant"] == variant and plan["nt"] == nt and plan["halo"][-1] == pad
                assert plan["halo"] == [(c["k"] - 1) * c["k"] ** i // 2 for i in range(c["layers"])] and max(plan["lds"]) <= 150 * 1024
                ends_n = (1 if head else 0) + (1 if tail else 0)
                assert plan["launches"] == (c["layers"] if variant == G.LAT else c["layers"] + ends_n)
                Ts = G.lengths_of(plan)
                assert set(Ts) == {1, 2, pad, pad + 1, nt - 1, nt, nt + 1, nt + pad + 1, 2 * nt + 3}
                blocks = lambda T: G.plan_of(pkg, c, variant, arith, T, head, tail)["grid"]
                assert blocks(nt) == (1, 4) and blocks(nt + 1) == (2, 4) and blocks(2 * nt + 3) == (3, 4)
                lens = sorted({n for T in Ts for n in G.ragged(T)})
                for edge in (nt, 2 * nt):
                    assert any(edge - 4 < n <= edge for n in lens) and any(edge < n <= edge + 4 for n in lens), (edge, lens)
                assert any(nt < n <= nt + pad for n in lens), "a sequence end inside the first block's right halo"
    if c in G.CASES:
        plan = G.plan_of(pkg, c, G.UNFUSED, G.F32, 1, 1, 1)
        assert plan["kernel"] == "dds_depthwise_kernel" and plan["nt"] == 64 and plan["launches"] == 3 * c["layers"] + 2


def test_every_instantiation_is_named_by_a_case(pkg):
    named = set()
    for c in G.CASES:
        for arith in (G.F32, G.F16, G.BF16):
            named |= set(G.expected_kernels(c, G.LAYER, arith))
        for head, tail in G.lat_ends(c):
            named |= set(G.expected_kernels(c, G.LAT, G.F32, head, tail))
            if c["layers"] > 2:
                named.add("dds_layer_lat_kernel<0, 0, %d>" % (6 if c["H"] <= 192 else 8))  # the layers between the first and the last
    assert named == LAYER_KERNELS | LAT_KERNELS, (LAYER_KERNELS | LAT_KERNELS) - named


def test_variant_0_is_the_engines_choice(pkg):
    c = G._case(192, 3, 3)
    assert G.plan_of(pkg, c, 0, G.F32, 128, batch=1)["variant"] == G.LAT  # 8 blocks of 16 tokens
    assert G.plan_of(pkg, c, 0, G.F32, 1537, batch=1)["variant"] == G.LAYER  # beyond 96 blocks
    assert G.plan_of(pkg, c, 0, G.F16, 128, batch=1)["variant"] == G.LAYER  # the latency kernel is fp32
    assert G.plan_of(pkg, G._case(16, 3, 3), 0, G.F32, 128, batch=1)["variant"] == G.UNFUSED  # the tiny model
    assert G.plan_of(pkg, G._case(192, 3, 1), 0, G.F32, 128, batch=1)["variant"] == G.UNFUSED  # Engine::run_dds fuses from two layers on


@pytest.mark.parametrize("r", G.REFUSALS, ids=G.refusal_id)
def test_dds_refusals_come_back_without_a_gpu(pkg, r):
    G.check_refusal(pkg, r, run_op=True)


def test_the_lds_limit_without_a_gpu(pkg):
    G.test_the_lds_limit_comes_from_the_plan_query(pkg)


def test_bad_arguments_are_refused_before_any_device_call(pkg):
    c = G._case(64, 3, 3)
    P = G.params_of(c)
    x = np.zeros((2, 64, 8), np.float32)
    args = (P["dw_w"], P["dw_b"], P["g1"], P["b1"], P["pw_w"], P["pw_b"], P["g2"], P["b2"])
    for kw, cause in ((dict(x=x, lens=[9, 1]), "lens[b] <= t"), (dict(x=x, lens=[-1, 1]), "lens[b] <= t"),
                      (dict(x=x, head_w=P["conv_w"], head_b=P["conv_b"], bias_rows=[0, 3]), "bias_rows[b] < n_bias_rows"),
                      (dict(x=x, variant=7), "variant 7")):
        with pytest.raises(pkg.VitsError) as e:
            pkg.op_dds_block(*args, **dict(dict(variant=G.UNFUSED), **kw))
        assert cause in str(e.value), str(e.value)


# ---- durations -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", S.DUR_COMBOS, ids=S.dur_id)
@pytest.mark.parametrize("ts", S.DUR_STRIDES)
def test_duration_inputs_stay_away_from_the_integers(ts, combo):
    """exp(logw) * scale in float64, on the fp32 inputs the kernel gets, is at least 0.04 from every integer: expf and the product in fp32 are good to a few ulp
    (2.4e-7 relative) of a value below 12, four orders of magnitude less, so ceil gives the same integer on both sides and no case is left out"""
    logw, row, lens, kw = S.dur_case(ts, combo)
    dur, cum, frames, sl, products = D.durations(logw[:, row], lens, **kw)
    assert len(lens) >= 4 and 1 in lens and max(lens) == ts
    if products.size:
        assert products.max() < 12.5 and np.abs(products - np.round(products)).min() >= 0.04
    else:
        assert combo.get("fixed")
    for b, n in enumerate(lens):
        assert np.isnan(logw[b, 0]).all() and np.isnan(logw[b, row, n:]).all()  # nothing but row `row` on [0, lens[b]) may be read
    assert sl.shape == (len(kw["stage_mul"]), len(lens)) and (cum[:, 0] == dur[:, 0]).all()
    if combo.get("ovr"):
        o = kw["overrides"]
        assert (o == -1).any() and (o > 0).any() and (o[3] == 0).all()
