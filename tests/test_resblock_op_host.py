"""vits_op_resblock without a GPU: the plan query (vits_op_resblock_plan, host arithmetic only) over the case table of tests/test_gpu_resblock_ops.py — imported, not
restated — proves that every case names the kernel it means and that its lengths really straddle that kernel's tile and segment edges; the refusals come back before
any device call; and a numpy emulation of one fused fp32 pair with two seeded defects shows that the edge-window rule of tests/split_ref.py catches what it is for."""
import numpy as np
import pytest

import split_ref as R
import test_gpu_resblock_ops as G


@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_every_case_names_its_kernel_and_its_lengths_straddle_the_edges(pkg, c):
    plan = G.plan_of(pkg, c, 1)
    assert plan["variant"] == c["variant"] and plan["kernel"].startswith(G.expected_kernel(c)), plan
    bo, S, halo = plan["bo"], plan["segment"], plan["halo"]
    assert bo > 0 and halo > 0 and plan["launches"] == (len(c["dils"]) if c["variant"] == G.PAIRS else 1)
    Ts = G.lengths_of(plan, c["variant"])
    assert {1, 2, 5, bo - 1, bo, bo + 1, bo + halo + 1, 2 * bo + 3} <= set(Ts)
    if c["variant"] == G.SEGMENTS:
        assert plan["tiles"] == c["tiles"] >= 2 and S == bo + (c["tiles"] - 1) * plan["advance"] and plan["advance"] > bo
        assert {S - 1, S + 1, 2 * S + 2} <= set(Ts)
    else:
        assert S == bo == plan["advance"]
    if c["nr"]:
        assert plan["nr"] == c["nr"]
    # the grid agrees: one more column than a block owns is one more block
    blocks = lambda T: G.plan_of(pkg, c, T)["grid"][0]
    assert blocks(S) == 1 and blocks(S + 1) == 2 and blocks(2 * S) == 2 and blocks(2 * S + 2) == 3
    assert G.plan_of(pkg, c, S + 1)["grid"][1] == 4
    if c["variant"] == G.SEGMENTS:  # a second tile of the first segment, not a second block
        assert blocks(bo + 1) == 1
    # the largest staged tensor stays small (C = 256 at ~250 columns, C = 32 at ~2.2 k)
    assert 4 * c["C"] * max(Ts) * 4 <= 4 << 20, (c, max(Ts))


def test_forced_column_tiles_and_segments_do_not_depend_on_the_grid(pkg):
    """forcing goes through the call: the same instantiation at one column and at a grid of thousands of blocks, where the planner by itself would switch"""
    for T, B in ((1, 1), (100000, 64)):
        for nr in (4, 2):
            c = G._case(G.F16, 256, 3, (1,), G.PAIRS, nr=nr)
            assert G.plan_of(pkg, c, T, batch=B)["kernel"] == "rbpair16_kernel<3, 1, 256, %d, false, true>" % nr
        c = G._case(G.F16, 64, 11, G.D135, G.BLOCK)
        assert G.plan_of(pkg, c, T, batch=B)["kernel"] == "rbblock16_kernel<11, 64, 4, 3, 1, 1, 3, 5, false, false>"
        c = G._case(G.BF16, 32, 3, G.D135, G.SEGMENTS, tiles=3)
        assert G.plan_of(pkg, c, T, batch=B)["kernel"] == "rbblock16_kernel<3, 32, 4, 3, 1, 1, 3, 5, true, true>"
    # the planner's own choice does switch with the grid
    auto = G._case(G.F16, 256, 3, (1,), G.PAIRS)
    assert G.plan_of(pkg, auto, 100, batch=1)["nr"] == 2 and G.plan_of(pkg, auto, 100000, batch=64)["nr"] == 4


def test_the_ragged_batch_puts_the_sequence_end_on_every_residue_mod_4():
    for T in (4, 5, 249, 250, 1104):
        assert sorted(n % 4 for n in G.ragged(T)) == [0, 1, 2, 3]
    assert G.ragged(1) == [1, 1, 1, 1] and G.ragged(2) == [2, 1, 1, 1]


@pytest.mark.parametrize("r", G.REFUSALS, ids=G.refusal_id)
def test_refusals_come_back_without_a_gpu(pkg, r):
    G.check_refusal(pkg, r, run_op=True)


# ---- a fused fp32 pair in numpy, with the two defects the edge windows are for --------------------------------------------------------------------------------
def emulate_pair(x, w1, b1, w2, b2, lens, dil, slope, bo, defect=None):
    """y = x + b2 + conv2(t), t = lrelu(b1 + conv1(lrelu(x))) zero outside [0, len), fp32 matrix products. defect "unmasked": t is not zeroed past the sequence end
    (conv 1 ran on the zero-padded input there); defect "halo": the outputs of the first tile read a zero where the first column of their right halo is."""
    C, _, k = w1.shape
    P1, P2 = (k - 1) * dil // 2, (k - 1) // 2

    def conv(w, a, step, n_out):  # output column o reads a[:, o + j step]
        A = np.stack([a[:, j * step: j * step + n_out] for j in range(k)], axis=1).reshape(C * k, n_out)
        return w.reshape(C, -1) @ A

    out = np.zeros_like(x)
    for b, n in enumerate(lens):
        a = np.zeros((C, n + 2 * (P1 + P2)), np.float32)
        a[:, P1 + P2: P1 + P2 + n] = R.lrelu32(x[b, :, :n], slope)
        t = R.lrelu32(conv(w1, a, dil, n + 2 * P2) + b1[:, None], slope)  # columns -P2 .. n + P2
        t[:, :P2] = 0
        if defect != "unmasked":
            t[:, P2 + n:] = 0
        y = R.epilogue32(conv(w2, t, 1, n), b2, x[b, :, :n])
        if defect == "halo" and n > bo:
            t[:, P2 + bo] = 0
            y[:, :bo] = R.epilogue32(conv(w2, t, 1, n), b2, x[b, :, :n])[:, :bo]
        out[b, :, :n] = y
    return out


@pytest.mark.parametrize("C,k,dil", [(32, 3, 1), (32, 7, 3), (64, 11, 5)])
def test_the_edge_window_rule_catches_an_unmasked_intermediate_and_a_missing_halo_column(pkg, C, k, dil):
    c = G._case(G.F32, C, k, (dil,), G.PAIRS)
    plan = G.plan_of(pkg, c, 1)
    bo = plan["bo"]
    T = bo + plan["halo"] + 1
    lens = G.ragged(T)
    x, w1, b1, w2, b2 = R.make_pair(C, k, dil, T, len(lens))
    ref, chain, rows = R.pair_reference(x, w1, b1, w2, b2, lens, dil, G.SLOPE)
    mask = R.edge_columns(lens, k, bo)
    assert 0 < mask.sum() <= len(lens) * 3 * (k - 1)
    ratios = {}
    for defect in (None, "unmasked", "halo"):
        got = emulate_pair(x, w1, b1, w2, b2, lens, dil, G.SLOPE, bo, defect)
        cols = R.gather_cols(got, lens)
        pool = R.EdgePool()
        pool.add(cols, ref, chain, rows, mask)
        ratios[defect] = pool.ratio()
        print("C%d k%d d%d %s: edge windows %.3g x the chain; overall rms %.2e of RMS (chain %.2e)" % (
            C, k, dil, defect, pool.ratio(), R.rms_err(cols, ref)[0], R.rms_err(chain, ref[rows])[0]))
    assert ratios[None] <= R.FACTOR, ratios
    assert ratios["unmasked"] > 100 * R.FACTOR and ratios["halo"] > 100 * R.FACTOR, ratios
