"""vits_op_flow_coupling without a GPU: the plan query (vits_op_flow_coupling_plan, host arithmetic only) over the case table of tests/test_gpu_flow_ops.py —
imported, not restated — proves that every case names the kernel it means, that its geometry is the launch-plan tables', and that its lengths really straddle that
kernel's block edges; the refusals come back before any device call; and a numpy emulation of the coupling layer with four seeded faults a tiled kernel could make
shows that the 2x rule of tests/flow_ref.py on the update m = x1' - x1 catches them while an un-faulted, reordered fp32 computation passes."""
import os
import re

import numpy as np
import pytest

import flow_ref as FR
import split_ref as R
import test_gpu_flow_ops as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plan_table.txt")


def golden_kernels():
    """{kernel name: {(block, lds)}} of every WaveNet / coupling row of the golden launch-plan table"""
    out = {}
    with open(GOLDEN) as f:
        for line in f:
            if line.startswith(("WN ", "FC ")):
                for name, _, _, _, block, lds in re.findall(r"((?:wavenet32|wavenet16|flow_couple16)_kernel<[^>]*>) \| (\d+) (\d+) (\d+) (\d+) (\d+)", line):
                    out.setdefault(name, set()).add((int(block), int(lds)))
    return out


@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_every_case_names_its_kernel_and_its_lengths_straddle_the_edges(pkg, c):
    plan = G.plan_of(pkg, c, 1)
    assert plan["variant"] == c["variant"] and plan["kernel"] == G.expected_kernel(c), plan
    # the name is one the launch-plan tables print (their 16-bit rows are the f16 instantiations), with the same block and LDS bytes
    table = golden_kernels()
    assert (plan["block"], plan["lds"]) in table[plan["kernel"].replace("true", "false")], (plan, table.get(plan["kernel"]))
    bo, halo = plan["bo"], plan["halo"]
    if c["variant"] == G.WAVENET:  # launch_plan.h: kWaveNetBM, one k = 5 halo
        assert (bo, halo, plan["launches"], plan["nct"]) == (64, 2, G.LAYERS + 2, 0) and plan["ncw"] == c["ncw"]
    else:  # flow_couple16_geom: 32 nct frames staged, four k = 5 halos per side
        assert (bo, halo, plan["launches"]) == (32 * c["nct"] - 16, 8, 1) and (plan["ncw"], plan["nct"]) == (c["ncw"], c["nct"])
        assert plan["block"] == 64 * 6 * c["nct"] // c["ncw"]
    Ts = G.lengths_of(plan)
    assert {1, 2, 5, bo - 1, bo, bo + 1, bo + halo + 1, 2 * bo + 3} == set(Ts) and max(Ts) <= 131
    # the grid agrees: one more column than a block owns is one more block; a length on each side of both edges the lengths reach
    blocks = lambda T: G.plan_of(pkg, c, T)["grid"][0]
    assert blocks(bo) == 1 and blocks(bo + 1) == 2 and blocks(2 * bo) == 2 and blocks(2 * bo + 3) == 3
    assert G.plan_of(pkg, c, bo + 1)["grid"][1] == 4
    lens = sorted({n for T in Ts for n in G.ragged(T)})
    for edge in (bo, 2 * bo):
        assert any(n <= edge for n in lens if n > edge - 4) and any(n > edge for n in lens if n <= edge + 4), (edge, lens)
    assert any(bo < n <= bo + halo for n in lens), "a sequence end inside the first block's halo"


def test_forced_tiles_do_not_depend_on_the_grid(pkg):
    """forcing goes through the call: the same instantiation at one frame and at a grid of thousands of blocks, where the planner by itself switches"""
    for T, B in ((1, 1), (100000, 64)):
        for ncw, nct in ((1, 1), (1, 2), (2, 2)):
            assert G.plan_of(pkg, G._case(G.F16, G.COUPLING, ncw, nct), T, batch=B)["kernel"] == "flow_couple16_kernel<false, %d, %d>" % (ncw, nct)
        for ncw in (1, 2):
            assert G.plan_of(pkg, G._case(G.BF16, G.WAVENET, ncw), T, batch=B)["kernel"] == "wavenet16_kernel<192, 5, true, %d>" % ncw
    auto = G._case(G.F16, G.COUPLING)
    assert G.plan_of(pkg, auto, 100, batch=1)["nct"] == 1 and G.plan_of(pkg, auto, 100000, batch=64)["nct"] == 2
    # variant 0: the fused fp32 layers from 384 blocks of 32 frames on
    f32 = G._case(G.F32, 0)
    assert G.plan_of(pkg, f32, 32 * 96 - 32, batch=4)["variant"] == G.UNFUSED and G.plan_of(pkg, f32, 32 * 96, batch=4)["variant"] == G.WAVENET


def test_the_ragged_batch_puts_the_sequence_end_on_every_residue_mod_4():
    for T in (4, 5, 63, 64, 131):
        assert sorted(n % 4 for n in G.ragged(T)) == [0, 1, 2, 3]
    assert G.ragged(1) == [1, 1, 1, 1] and G.ragged(2) == [2, 1, 1, 1]


@pytest.mark.parametrize("r", G.REFUSALS, ids=G.refusal_id)
def test_refusals_come_back_without_a_gpu(pkg, r):
    G.check_refusal(pkg, r)


def test_bad_lens_and_speaker_rows_are_refused_before_any_device_call(pkg):
    W = FR.make_weights()
    z = np.zeros((2, 2 * FR.HALF, 8), np.float32)
    args = (z, W["w_pre"], W["b_pre"], W["w_in"], W["b_in"], W["w_rs"], W["b_rs"], W["w_post"], W["b_post"])
    for kw, cause in ((dict(lens=[9, 1]), "lens[b] <= t"), (dict(lens=[-1, 1]), "lens[b] <= t"), (dict(bias_rows=[0, 3]), "bias_rows[b] < n_bias_rows"),
                      (dict(bias_rows=[-1, 0]), "bias_rows[b] < n_bias_rows")):
        with pytest.raises(pkg.VitsError) as e:
            pkg.op_flow_coupling(*args, variant=G.UNFUSED, **kw)
        assert cause in str(e.value), str(e.value)


# ---- the coupling layer in numpy as a tiled kernel would compute it, with the faults the rule is for ---------------------------------------------------------
def emulate_layer(x0, x1, W, lens, bias_rows, bo, fault=None):
    """x1' [B, HALF, T] by fp32 matrix products (the BLAS order: an accumulation order that is neither the chain's nor the reference's), utterance by utterance.
    Faults, each in ONE layer: "halo": the outputs of the first block read a zero where the first column of their right halo of h is (layer 1);
    "unmasked": h is not zeroed behind the sequence end — the pre conv's bias stands there (layer 0); "tap": one tap of one 32-channel chunk is dropped
    (layer 2); "last_rs": the last layer's rs is added to h instead of out."""
    H, K, L = FR.H, FR.K, FR.LAYERS
    P = (K - 1) // 2
    out_x1 = np.zeros_like(x1)

    def gated(w, hp, n):  # hp: h with P columns of padding on either side
        A = np.stack([hp[:, j:j + n] for j in range(K)], axis=1).reshape(H * K, n)
        return w.reshape(2 * H, -1) @ A

    for b, n in enumerate(lens):
        h = (W["w_pre"][:, :, 0] @ x0[b, :, :n] + W["b_pre"][:, None]).astype(np.float32)
        out = np.zeros_like(h)
        for l in range(L):
            hp = np.zeros((H, n + 2 * P), np.float32)
            hp[:, P:P + n] = h
            if fault == "unmasked" and l == 0:
                hp[:, P + n:] = W["b_pre"][:, None]
            w = W["w_in"][l]
            if fault == "tap" and l == 2:
                w = w.copy()
                w[:, 32:64, 3] = 0
            g = gated(w, hp, n)
            if fault == "halo" and l == 1 and n > bo:
                hp[:, P + bo] = 0
                g[:, :bo] = gated(w, hp, n)[:, :bo]
            a = FR.gate32(g + W["b_in"][bias_rows[b], l][:, None])
            rs = (W["w_rs"][l][:, :, 0] @ a + W["b_rs"][l][:, None]).astype(np.float32)
            if l + 1 < L:
                h, out = h + rs[:H], out + rs[H:]
            elif fault == "last_rs":
                h = h + rs
            else:
                out = out + rs
        out_x1[b, :, :n] = x1[b, :, :n] + (W["w_post"][:, :, 0] @ out + W["b_post"][:, None]).astype(np.float32)
    return out_x1


@pytest.mark.parametrize("hot", [False, True], ids=["unit", "hot"])
def test_the_rule_on_the_update_catches_what_a_tiled_kernel_could_get_wrong(pkg, hot):
    """Every fault exceeds the 2x bound on the edge-window pool (the two edge faults) or overall (the two that touch every column), on both draws; the un-faulted
    BLAS-order computation stays under it on both figures. Measured: un-faulted 0.87-0.93 x the chain; the faults 2.9e3 x (the unmasked padding on the hot draw, overall) to
    8e5 x. No fault needed a smaller window than the one the GPU test pools over."""
    plan = G.plan_of(pkg, G.CASES[0], 1)
    bo = plan["bo"]
    T = bo + plan["halo"] + 1
    lens = G.ragged(T)
    W = FR.make_weights()
    x0, x1 = FR.make_inputs(T, hot)
    m64, m32, x1c = FR.layer_reference(x0, x1, W, lens, FR.BIAS_ROWS)
    mask = R.edge_columns(lens, FR.K, bo)
    assert 0 < mask.sum() <= len(lens) * 3 * (FR.K - 1)
    edge, overall = {}, {}
    for fault in (None, "halo", "unmasked", "tap", "last_rs"):
        m = FR.update_of(emulate_layer(x0, x1, W, lens, FR.BIAS_ROWS, bo, fault), x1c, lens)
        pool = R.EdgePool()
        pool.add(m, m64, m32, np.arange(FR.HALF), mask)
        g, ch = FR.ratios(m, m64, m32)
        edge[fault], overall[fault] = pool.ratio(), g / ch
        print("%s %s: %.3g x the chain overall, %.3g x on the edge windows (chain %.2e of RMS)" % ("hot" if hot else "unit", fault, g / ch, pool.ratio(), ch))
    assert edge[None] <= FR.FACTOR and overall[None] <= FR.FACTOR, (edge, overall)
    assert edge["halo"] > 100 * FR.FACTOR and edge["unmasked"] > 100 * FR.FACTOR, edge
    assert overall["tap"] > 100 * FR.FACTOR and overall["last_rs"] > 100 * FR.FACTOR, overall
