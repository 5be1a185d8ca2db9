"""Ragged batches on the lists of existing tiles (tile_map.h), at operator level: every converted kernel run over its list (VITS_TILE_MAP=1) gives the bits of
its dense grid (VITS_NO_TILE_MAP=1), and writes nothing behind an utterance's end.

Through the vits_op_* entry points, which read the two knobs at every call. A batch of six utterances with the lengths {0, 1, w - 1, w, w + 1, 2 w + 5}
relative to the kernel's own tile width w, and a batch of one whose dense grid has a tile more than the utterance. vits_op_tile_map_launches counts the
launches that were ISSUED over a list: every test states how many its operator makes. The convolutions run lists on the throughput tiles only
(conv_tile_mapped), which the planner gives large grids: their shapes here have few input channels and many rows (>= 512 blocks of 128 x 128, >= 1024 for
the transposed conv's two taps); the grouped launch always runs on that tile. Outputs are staged as 0xFF bytes (vits_op_set_output_fill; the grouped
operator always): behind an utterance's end every word must still be 0xFFFFFFFF, so a stray store of any value, zero included, shows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = 0xFFFFFFFF


@pytest.fixture
def nan_outputs(pkg):
    pkg.op_set_output_fill(0xFF)
    yield
    pkg.op_set_output_fill(0)


def both_forms(pkg, monkeypatch, run, launches):
    """run() under VITS_NO_TILE_MAP=1 and under VITS_TILE_MAP=1: no launch over a list in the first, exactly `launches` in the second"""
    out = {}
    for knob, other in (("VITS_NO_TILE_MAP", "VITS_TILE_MAP"), ("VITS_TILE_MAP", "VITS_NO_TILE_MAP")):
        monkeypatch.delenv(other, raising=False)
        monkeypatch.setenv(knob, "1")
        n0 = pkg.op_tile_map_launches()
        out[knob] = (run(), pkg.op_tile_map_launches() - n0)
    monkeypatch.delenv("VITS_TILE_MAP", raising=False)
    (dense, nd), (listed, nl) = out["VITS_NO_TILE_MAP"], out["VITS_TILE_MAP"]
    assert nd == 0 and nl == launches, (nd, nl, launches)
    return dense, listed


def six(w):
    return np.array([0, 1, w - 1, w, w + 1, 2 * w + 5], np.int32)


def check(dense, listed, lens, len_out=None):
    """[B, C, T] outputs: the same bits; the sentinel in every word behind the utterance's end; numbers in front of it"""
    len_out = lens if len_out is None else len_out
    assert np.array_equal(dense.view(np.uint32), listed.view(np.uint32))
    for b, n in enumerate(len_out):
        assert (listed[b, :, n:].view(np.uint32) == SENTINEL).all(), b
        assert np.isfinite(listed[b, :, :n]).all() and (n == 0 or listed[b, :, :n].any()), b


def batches(w, big):
    """(lens, t): the six lengths, and a batch of one (long enough for a large grid where the planner asks for one) whose grid has a tile past its end"""
    yield six(w), 2 * w + 5
    yield np.array([big - w - 2], np.int32), big


@pytest.mark.parametrize("kind", ["standard", "residual_accumulate_scale"])
def test_conv_mfma_on_lists(pkg, monkeypatch, nan_outputs, kind):
    rng = np.random.default_rng(11)
    cin, cout, w = 32, 4096, 128  # rows % 128 == 0 and 3 x 32 x 6 = 576 blocks: the 128 x 128 tile
    k, dil = (7, 1) if kind == "standard" else (11, 3)
    wt = (rng.standard_normal((cout, cin, k)) * 0.05).astype(np.float32)
    bias = rng.standard_normal(cout).astype(np.float32)
    for lens, t in batches(w, 16 * w + 5):
        B = len(lens)
        x = rng.standard_normal((B, cin, t)).astype(np.float32)
        extra = {}
        if kind != "standard":
            extra = dict(residual=rng.standard_normal((B, cout, t)).astype(np.float32), accum=rng.standard_normal((B, cout, t)).astype(np.float32), out_scale=1.0 / 3.0)
        dense, listed = both_forms(pkg, monkeypatch, lambda: pkg.op_conv1d(x, wt, bias, dilation=dil, pre_slope=0.1, lens=lens, **extra), 1)
        check(dense, listed, lens)


def test_transposed_conv_on_lists(pkg, monkeypatch, nan_outputs):
    rng = np.random.default_rng(12)
    cin, cout, s, w = 32, 1024, 8, 128  # 8192 rows: 3 x 64 x 6 = 1152 blocks of 128 x 128; the columns of an utterance are len + 1
    wt = (rng.standard_normal((cin, cout, 2 * s)) * 0.05).astype(np.float32)
    bias = rng.standard_normal(cout).astype(np.float32)
    for lens, t in batches(w, 16 * w + 5):
        x = rng.standard_normal((len(lens), cin, t)).astype(np.float32)
        dense, listed = both_forms(pkg, monkeypatch, lambda: pkg.op_conv_transpose1d(x, wt, bias, s, 0, pre_slope=0.1, lens=lens), 1)
        check(dense, listed, lens, [s * n + s if n else 0 for n in lens])


@pytest.mark.parametrize("C,k,variant", [(32, 11, "pairs"), (64, 7, "pairs"), (128, 3, "pairs"), (32, 3, "block"), (64, 3, "block")])
def test_fused_resblock_kernels_on_lists(pkg, monkeypatch, nan_outputs, C, k, variant):
    rng = np.random.default_rng(13)
    v = pkg.RB_VARIANT_PAIRS if variant == "pairs" else pkg.RB_VARIANT_BLOCK
    dils = [1, 3, 5]
    w = pkg.op_resblock_plan(C, k, dils, 1000, batch=6, variant=v)["bo"]  # rbpair32_kernel<k, d, C> / rbblock32_kernel<C>: output columns per block
    w1, w2 = ((rng.standard_normal((3, C, C, k)) * (0.5 / np.sqrt(C * k))).astype(np.float32) for _ in range(2))
    b1, b2 = (rng.standard_normal((3, C)).astype(np.float32) * 0.1 for _ in range(2))
    for lens, t in batches(w, 2 * w + 5):
        B = len(lens)
        x = rng.standard_normal((B, C, t)).astype(np.float32)
        acc = rng.standard_normal((B, C, t)).astype(np.float32)
        dense, listed = both_forms(pkg, monkeypatch, lambda: pkg.op_resblock(x, w1, b1, w2, b2, dils, 0.1, variant=v, accum=acc, out_scale=1.0 / 3.0, lens=lens, t=t),
                                   3 if variant == "pairs" else 1)  # one launch per pair / one for the resblock
        check(dense, listed, lens)


@pytest.mark.parametrize("taps", [(3, 7, 11), (11, 7, 3), (11, 3), (7, 11), (3, 7)], ids=lambda t: "k" + "_".join(map(str, t)))
@pytest.mark.parametrize("dil", [1, 5])
def test_grouped_launch_on_lists(pkg, monkeypatch, taps, dil):
    """conv_group_list_kernel against conv_group_kernel: three members and two (every absent slot), members given in any order, ONE launch over the
    concatenated lists — and each member against its own single launch (op_conv1d on the dense grid), so that an entry read from another member's list shows"""
    rng = np.random.default_rng(14)
    C, w, n = 128, 128, len(taps)
    ws = [(rng.standard_normal((C, C, k)) * (0.5 / np.sqrt(C * k))).astype(np.float32) for k in taps]
    bias = rng.standard_normal((n, C)).astype(np.float32) * 0.1
    for lens, t in batches(w, 2 * w + 5):
        B = len(lens)
        x = rng.standard_normal((n, B, C, t)).astype(np.float32)
        dense, listed = both_forms(pkg, monkeypatch, lambda: pkg.op_conv_group(x, ws, bias, dil, 0.1, lens=lens), 1)
        for i in range(n):
            check(dense[i], listed[i], lens)
            monkeypatch.setenv("VITS_NO_TILE_MAP", "1")
            y = pkg.op_conv1d(x[i], ws[i], bias[i], dilation=dil, pre_slope=0.1, lens=lens)  # (zeros behind the ends: compared in front of them)
            monkeypatch.delenv("VITS_NO_TILE_MAP")
            for b, m in enumerate(lens):
                single = np.maximum(y[b, :, :m], 0.1 * y[b, :, :m])  # the member stores leaky_relu of the conv's result (the engine's first conv of a pair)
                assert np.array_equal(single, listed[i][b, :, :m]), (i, b)
