"""The DDS block of the stochastic duration predictor at operator level (vits_op_dds_block): the three launches per layer (dds_depthwise_kernel, the 1x1
conv, add_layer_norm_kernel), the fused dds_layer_kernel<ARITH, MAXCH> and the latency kernel dds_layer_lat_kernel<HEAD, TAIL, MAXCH> with its fused heads
(pointwise_from1_kernel's 1 -> H conv plus conditioning; an H -> H 1x1 conv with a per-utterance bias row) and tail (a 1x1 projection), on shapes no whole
model of the suite has: every channel count the planner accepts a kernel build for, other tap counts and layer counts, sequence ends on every tile and halo edge.

CASES lists the blocks (channels, k, layers; dilation k^i). vits_op_dds_block_plan names the instantiation a (case, variant, arithmetic, head, tail) runs, its
tokens per block NT and each layer's halo; the lengths of a case come from those (lengths_of): {1, 2, pad, pad + 1, NT - 1, NT, NT + 1, NT + pad + 1, 2 NT + 3}
with pad the last layer's halo, as the batch lens = [T, T - 1, T - 2, T - 3] (clipped at 1). Data: tests/dp_ref.py.

Which case names which instantiation (every one of them runs in a passing test below):
  dds_layer_kernel<A, 2>      A = 0, 1, 2 (fp32, bf16, fp16): 32-k3-l3, 64-k3-l3, 64-k5-l2       dds_layer_kernel<A, 4>: 96-k3-l3
  dds_layer_kernel<A, 6>      160-k3-l3, 192-k3-l3, 192-k5-l2, 192-k7-l2, 192-k9-l1               dds_layer_kernel<A, 8>: 224-k3-l3, 256-k3-l2, 256-k3-l1
  dds_layer_lat_kernel<0, 0, 6>, <1, 0, 6>, <2, 0, 6>, <0, 1, 6>: 32-k3-l3, 64-k3-l3, 64-k5-l2, 192-k3-l3, 192-k5-l2, 192-k7-l2 with every head / tail
      (the head sits in the first layer's kernel, the tail in the last one's); <0, 0, 6> also 96-k3-l3 and 160-k3-l3
  dds_layer_lat_kernel<1, 1, 6>, <2, 1, 6>: 192-k9-l1 (one layer carries head and tail), and <0, 0, 6>, <1, 0, 6>, <2, 0, 6>, <0, 1, 6> again
  dds_layer_lat_kernel<0, 0, 8>, <1, 0, 8>, <2, 0, 8>, <0, 1, 8>: 256-k3-l2 (and <0, 0, 8>, <0, 1, 8>: 224-k3-l3)
  dds_layer_lat_kernel<1, 1, 8>, <2, 1, 8>: 256-k3-l1
(tests/test_dp_op_host.py derives the same table from CASES and checks that it is complete.) 256 channels run two layers here: dds_depthwise_kernel's 64-token
tile has no room for 256 channels at dilation 9 (157696 bytes of LDS against 153600) and the launcher refuses, so a three-layer block of 256 channels exists on
the fused kernels only. WIDE_CASES holds dds_layer_kernel to float64 directly there (three layers, and four: dilation 27, 150528 bytes), and the latency kernel
to dds_layer_kernel bit for bit.

What is asserted:
  * the plan query names the kernel that was asked for;
  * bit identity, no tolerance, on every valid column at every length: variant 2 == variant 1 in fp32, fp16 and bf16; variant 3 == variant 1 in fp32 for
    every head / tail combination; with head 2, each utterance's bias row == a call whose one-row table holds that row;
  * fp32 anchor: variant 1 against dp_ref.dds_block in float64 under the 2x rule of tests/split_ref.py, the yardstick being dp_ref.dds_block in float32 on the
    same data — pooled over the case (asserted), per length (asserted from 8192 outputs on, printed below that, where the ratio of two rms errors is noise), per
    32-channel row group pooled over the lengths (asserted from 8192 outputs on), and pooled on the edge windows (the last `pad` columns of every utterance, `pad`
    columns on each side of every 16-token block boundary: the finest tile of the three families). With heads and tail at 64 and 192 channels, on y2.
    The variants 2 and 3 are held to the same float64 result through their bit identity with variant 1 at the same lengths.
  * 16-bit arithmetics: bit identity with variant 1 and hygiene only. A rounding flip of a 16-bit intermediate dominates any ratio of two accumulation orders
    (tests/test_gpu_resblock_ops.py and tests/test_gpu_flow_ops.py measured the same and chose the same).
  * hygiene, per kernel family at T = NT + 5: results finite, nothing written behind lens[b] (the op stages NaNs there and returns them), a lens = 0 row
    untouched, every row == its batch-1 call, a t_stride far larger than t and one that is no multiple of 4 give the same bits, with a tail variant 3 writes no y,
    and the latent row zc does not name is not read (it is staged as NaN);
  * refusals name their cause, from the plan query and from the op alike: 16 and 288 channels, k = 2 at dilation 1, a layer whose tile passes the LDS limit,
    16-bit arithmetic on the latency kernel, more tail rows than channels.

The 32-channel cases of test_latency_kernel_equals_three_launches fail on the commit before this file: dds_layer_lat_kernel launches channels / 16 waves, 128
threads at 32 channels, and its LayerNorm statistics were written by the threads tid < 256 only, so groups 8..15 of the 16 partial sums were never written and
all 16 were read. There (this file and the operator on top of the parent's stage1_lat.hip) all six cases 32-k3-l3 fail their first bit-identity assertion, at
T = 1: every value of utterance 0 differs from the three launches', by up to 2.8 (head 0, tail 0), 1.2 (0, 1), 2.0 (1, 0), 2.1 (1, 1) on outputs of unit size,
and the result is NaN with head 2 (whatever the unwritten LDS held). The kernel's threads now walk the 16 groups; blocks of 256 threads and more compute the
same floats as before (every other case here, and the model-level bit-identity tests, say so).

Observed on an MI355X, on the commit that adds this file (the tests print every figure): the fp32 restatement's error is 1.4e-7 (32 channels) to 3.0e-7
(256 channels, four layers) of the RMS of the result, 2.1e-7 to 4.4e-7 with head and tail on y2. GPU / restatement, pooled per case: 0.91 to 0.94 without
heads, 0.94 to 0.97 with head and tail; edge windows 0.91 to 0.97; per 32-channel row group (34528 to 46752 outputs each) 0.89 to 0.98; per length from
8192 outputs on 0.91 to 0.95; below that 0.8 to 1.6 (1.59: 256-k3-l4 at T = 1, 1024 outputs), printed and not asserted. Every bit-identity and hygiene
assertion holds in fp32, fp16 and bf16. The whole file runs in 5 s."""
import numpy as np
import pytest

import dp_ref as D
import split_ref as R

pytestmark = pytest.mark.gpu
F32, BF16, F16 = 0, 1, 2  # pkg.ARITH_*
ARITH_NAME = {F32: "f32", F16: "f16", BF16: "bf16"}
UNFUSED, LAYER, LAT = 1, 2, 3  # pkg.DDS_VARIANT_*
NAN_BITS = 0xFFFFFFFF  # what the op stages behind lens[b]
BIAS_ROWS = [2, 0, 1, 2]
LAT_NT = 16


def _case(H, k, layers):
    return dict(H=H, k=k, layers=layers)


# the model's shape (k = 3, three layers) at every channel count with a kernel build of its own; k = 5; H k > 1024 (the parameter tail loop of dds_layer_kernel);
# H k > 2 x block with one layer (the same loop of the latency kernel, and the only way to one kernel with head and tail); one layer at MAXCH = 8
# (256 channels: two layers. dds_depthwise_kernel's 64-token tile has no room for dilation 9 there, so the three launches do not exist for three layers:
# WIDE_CASES below holds those to float64 through dds_layer_kernel instead, and the two fused families to each other)
CASES = [_case(H, 3, 3) for H in (32, 64, 96, 160, 192, 224)] + [_case(256, 3, 2), _case(64, 5, 2), _case(192, 5, 2), _case(192, 7, 2), _case(192, 9, 1), _case(256, 3, 1)]
WIDE_CASES = [_case(256, 3, 3), _case(256, 3, 4)]  # (four layers: dilation 27, 150528 of the 153600 bytes dds_layer_kernel may ask for)
# every head / tail combination of the latency kernel where the issue asks for all six instantiations per MAXCH, the plain layer and one tail elsewhere
ALL_ENDS = [(h, t) for h in (0, 1, 2) for t in (0, 1)]
LAT_ENDS = {H: ALL_ENDS for H in (32, 64, 192, 256)}
MAXCH_LAYER = {32: 2, 64: 2, 96: 4, 128: 4, 160: 6, 192: 6, 224: 8, 256: 8}


def case_id(c):
    return "%d-k%d-l%d" % (c["H"], c["k"], c["layers"])


def lat_ends(c):
    return LAT_ENDS.get(c["H"], [(0, 0), (0, 1)])


def tail_rows_of(c, head, tail):
    """the predictor's arrangement behind an H -> H head is an H -> H projection; a conv flow projects to 3 x 10 bins - 1 = 29 rows"""
    return 0 if not tail else c["H"] if head == 2 else 29


def expected_kernels(c, variant, arith, head=0, tail=0):
    """(first, last) layer's instantiation as the launch-plan tables print it"""
    if variant == LAYER:
        n = "dds_layer_kernel<%d, %d>" % (arith, MAXCH_LAYER[c["H"]])
        return n, n
    m = 6 if c["H"] <= 192 else 8
    one = c["layers"] == 1
    return "dds_layer_lat_kernel<%d, %d, %d>" % (head, tail if one else 0, m), "dds_layer_lat_kernel<%d, %d, %d>" % (head if one else 0, tail, m)


def plan_of(pkg, c, variant, arith, T, head=0, tail=0, batch=4):
    pkg.op_set_arith(arith)
    try:
        return pkg.op_dds_block_plan(c["H"], c["k"], c["layers"], T, batch=batch, variant=variant, head=head, tail_rows=tail_rows_of(c, head, tail))
    finally:
        pkg.op_set_arith(F32)


def lengths_of(plan):
    nt, pad = plan["nt"], plan["halo"][-1]
    return sorted({1, 2, pad, pad + 1, nt - 1, nt, nt + 1, nt + pad + 1, 2 * nt + 3})


def ragged(T):
    return [max(1, T - i) for i in range(4)]


def seed_of(c, T):
    return ((c["H"] * 131 + c["k"]) * 17 + c["layers"]) * 4099 + T


_params = {}


def params_of(c):
    key = case_id(c)
    if key not in _params:
        _params[key] = D.make_params(c["H"], c["k"], c["layers"], seed_of(c, 0), tail_rows=29)
        rng = np.random.default_rng(seed_of(c, 0) + 1)
        _params[key]["tail_w_sq"] = (rng.standard_normal((c["H"], c["H"])) / np.sqrt(c["H"])).astype(np.float16).astype(np.float32)
        _params[key]["tail_b_sq"] = (0.1 * rng.standard_normal(c["H"])).astype(np.float32)
    return _params[key]


def inputs_of(c, T, ts=None, B=4):
    """x, z, cond ~ N(0, 1) on [B, *, ts]; the same values at every ts"""
    rng = np.random.default_rng(seed_of(c, T))
    ts = T if ts is None else ts
    out = []
    for rows in (c["H"], 2, c["H"]):
        a = np.zeros((B, rows, ts), np.float32)
        a[:, :, :T] = rng.standard_normal((B, rows, T)).astype(np.float32)
        out.append(a)
    return out


def with_tail(P, c, head, tail):
    """the parameter set a (head, tail) runs with: the square projection behind head 2"""
    if tail and head == 2:
        P = dict(P, tail_w=P["tail_w_sq"], tail_b=P["tail_b_sq"])
    return P


def run(pkg, c, variant, arith, T, lens, head=0, tail=0, ts=None, bias_rows=BIAS_ROWS, inputs=None, conv_b=None, zc=0):
    """(y, y2) of vits_op_dds_block as the device holds them"""
    P = with_tail(params_of(c), c, head, tail)
    x, z, cond = inputs_of(c, T, ts, len(lens)) if inputs is None else inputs
    kw = dict(lens=lens, t=T, variant=variant)
    if head == 1:
        kw.update(z=z, cond=cond, zc=zc, head_w=P["from1_w"], head_b=P["from1_b"])
    elif head == 2:
        kw.update(x=x, head_w=P["conv_w"], head_b=P["conv_b"] if conv_b is None else conv_b, bias_rows=bias_rows)
    else:
        kw.update(x=x)
    if tail:
        kw.update(tail_w=P["tail_w"], tail_b=P["tail_b"])
    pkg.op_set_arith(arith)
    try:
        return pkg.op_dds_block(P["dw_w"], P["dw_b"], P["g1"], P["b1"], P["pw_w"], P["pw_b"], P["g2"], P["b2"], **kw)
    finally:
        pkg.op_set_arith(F32)


def result_of(out, tail):
    return out[1] if tail else out[0]


def same_valid_bits(a, b, lens, what):
    for i, n in enumerate(lens):
        ga, gb = a[i, :, :n].view(np.uint32), b[i, :, :n].view(np.uint32)
        if not np.array_equal(ga, gb):
            diff = np.argwhere(ga != gb)
            e = np.abs(a[i, :, :n].astype(np.float64) - b[i, :, :n])
            raise AssertionError("%s: utterance %d (len %d): %d of %d values differ, first at (channel, t) = %s, largest difference %.3e"
                                 % (what, i, n, len(diff), ga.size, tuple(diff[0]), np.nanmax(e) if np.isfinite(e).any() else float("nan")))


_unfused = {}


def unfused(pkg, c, arith, T, head, tail, variant=UNFUSED):
    """variant 1 at the ragged batch of T, once per (case, arithmetic, T, head, tail)"""
    key = (case_id(c), arith, T, head, tail, variant)
    if key not in _unfused:
        _unfused[key] = run(pkg, c, variant, arith, T, ragged(T), head, tail)
    return _unfused[key]


@pytest.mark.parametrize("arith", [F32, F16, BF16], ids=lambda a: ARITH_NAME[a])
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_fused_layer_equals_three_launches(pkg, c, arith):
    plan = plan_of(pkg, c, LAYER, arith, 1)
    assert plan["variant"] == LAYER and (plan["kernel"], plan["kernel_last"]) == expected_kernels(c, LAYER, arith) and plan["nt"] == 32, plan
    for T in lengths_of(plan):
        lens = ragged(T)
        got, _ = run(pkg, c, LAYER, arith, T, lens)
        want, _ = unfused(pkg, c, arith, T, 0, 0)
        same_valid_bits(got, want, lens, "%s %s T = %d: dds_layer_kernel against the three launches" % (case_id(c), ARITH_NAME[arith], T))


LAT_PARAMS = [(c, h, t) for c in CASES for h, t in lat_ends(c)]


@pytest.mark.parametrize("c,head,tail", LAT_PARAMS, ids=lambda v: case_id(v) if isinstance(v, dict) else str(v))
def test_latency_kernel_equals_three_launches(pkg, c, head, tail):
    plan = plan_of(pkg, c, LAT, F32, 1, head, tail)
    assert plan["variant"] == LAT and (plan["kernel"], plan["kernel_last"]) == expected_kernels(c, LAT, F32, head, tail) and plan["nt"] == LAT_NT, plan
    assert plan["launches"] == c["layers"] and plan["block"] == c["H"] * 4
    for T in lengths_of(plan):
        lens = ragged(T)
        got = result_of(run(pkg, c, LAT, F32, T, lens, head, tail), tail)
        want = result_of(unfused(pkg, c, F32, T, head, tail), tail)
        same_valid_bits(got, want, lens, "%s head %d tail %d T = %d: dds_layer_lat_kernel against the three launches" % (case_id(c), head, tail, T))


@pytest.mark.parametrize("variant,arith", [(UNFUSED, F32), (LAYER, F32), (LAYER, F16), (LAT, F32)], ids=["unfused-f32", "layer-f32", "layer-f16", "lat-f32"])
@pytest.mark.parametrize("c", [_case(64, 3, 3), _case(192, 3, 3)], ids=case_id)
def test_each_bias_row_is_the_call_with_that_row_alone(pkg, c, variant, arith):
    T = 21
    lens = ragged(T)
    table = params_of(c)["conv_b"]
    got = run(pkg, c, variant, arith, T, lens, head=2)[0]
    x, z, cond = inputs_of(c, T)
    for b, n in enumerate(lens):
        one = run(pkg, c, variant, arith, T, [n], head=2, bias_rows=None, inputs=(x[b:b + 1], z[b:b + 1], cond[b:b + 1]), conv_b=table[BIAS_ROWS[b]:BIAS_ROWS[b] + 1])[0]
        same_valid_bits(got[b:b + 1], one, [n], "%s variant %d: bias row %d of utterance %d" % (case_id(c), variant, BIAS_ROWS[b], b))
    other = run(pkg, c, variant, arith, T, lens, head=2, bias_rows=[0, 0, 0, 0])[0]
    assert not np.array_equal(got[0, :, :T], other[0, :, :T]), "the bias row is not used"


# ---- the fp32 anchor -----------------------------------------------------------------------------------------------------------------------------
class Pool:
    """squared errors of the GPU result and of the fp32 restatement against float64, and the reference's squares, summed over whatever is added"""

    def __init__(self):
        self.g = self.c = self.r = 0.0
        self.n = 0

    def add(self, got, chain, ref):
        ref = np.asarray(ref, np.float64)
        self.g += float(((np.asarray(got, np.float64) - ref) ** 2).sum())
        self.c += float(((np.asarray(chain, np.float64) - ref) ** 2).sum())
        self.r += float((ref ** 2).sum())
        self.n += ref.size

    def figures(self):
        """(gpu rms, restatement rms) relative to the reference's RMS"""
        return np.sqrt(self.g / self.r), np.sqrt(self.c / self.r)


def edge_mask(lens, pad, nt=LAT_NT):
    """columns (of the batch's valid columns side by side) within `pad` of a block boundary inside the utterance, or among its last `pad`"""
    out = []
    for n in lens:
        t = np.arange(n)
        m = t >= n - pad
        for edge in range(nt, n, nt):
            m |= (t >= edge - pad) & (t < edge + pad)
        out.append(m)
    return np.concatenate(out)


def anchor_lengths(pkg, c):
    """the lengths of both fused families: what variant 1 is held to float64 at is what their bit identity is asserted at"""
    out = set(lengths_of(plan_of(pkg, c, LAYER, F32, 1)))
    try:
        out |= set(lengths_of(plan_of(pkg, c, LAT, F32, 1)))
    except pkg.VitsError:
        pass  # (WIDE_CASES: four layers at 256 channels have no latency kernel)
    return sorted(out)


def hold_to_float64(pkg, c, head, tail, variant=UNFUSED):
    P = with_tail(params_of(c), c, head, tail)
    H, pad = c["H"], (c["k"] - 1) * c["k"] ** (c["layers"] - 1) // 2
    rows = P["tail_w"].shape[0] if tail else H
    label = "%s head %d tail %d" % (case_id(c), head, tail)
    whole, edges = Pool(), Pool()
    groups = [Pool() for _ in range((rows + 31) // 32)]
    for T in anchor_lengths(pkg, c):
        lens = ragged(T)
        x, z, cond = inputs_of(c, T)
        kw = dict(x=x, z=z, cond=cond, head=head, bias_rows=BIAS_ROWS, tail=bool(tail))
        ref = result_of(D.dds_block(P, lens, np.float64, **kw), tail)
        chain = result_of(D.dds_block(P, lens, np.float32, **kw), tail)
        got = R.gather_cols(result_of(unfused(pkg, c, F32, T, head, tail, variant), tail), lens)
        assert np.isfinite(got).all(), (label, T, "a slot past an utterance's length (NaN) was read")
        one = Pool()
        one.add(got, chain, ref)
        g, ch = one.figures()
        print("%s T = %d: %d outputs: gpu rms %.2e, fp32 restatement %.2e of RMS; ratio %.2f" % (label, T, got.size, g, ch, g / ch))
        if got.size >= R.MIN_ELEMS:
            assert g <= R.FACTOR * ch, (label, T, g, ch)
        whole.add(got, chain, ref)
        m = edge_mask(lens, pad)
        edges.add(got[:, m], chain[:, m], ref[:, m])
        for i, p in enumerate(groups):
            p.add(got[32 * i:32 * i + 32], chain[32 * i:32 * i + 32], ref[32 * i:32 * i + 32])
    g, ch = whole.figures()
    print("%s pooled: %d outputs: gpu rms %.2e, fp32 restatement %.2e of RMS; ratio %.2f" % (label, whole.n, g, ch, g / ch))
    assert g <= R.FACTOR * ch, (label, "pooled", g, ch)
    g, ch = edges.figures()
    print("%s edge windows: %d outputs: ratio %.2f" % (label, edges.n, g / ch))
    assert edges.n > 0 and g <= R.FACTOR * ch, (label, "edge windows", g, ch)
    ratios = []
    for i, p in enumerate(groups):
        g, ch = p.figures()
        ratios.append(g / ch)
        if p.n >= R.MIN_ELEMS:
            assert g <= R.FACTOR * ch, (label, "row group", i, g, ch)
    print("%s row groups (%d outputs each): ratios %s" % (label, groups[0].n, " ".join("%.2f" % v for v in ratios)))


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_three_launches_against_float64(pkg, c):
    hold_to_float64(pkg, c, 0, 0)


@pytest.mark.parametrize("head", [1, 2])
@pytest.mark.parametrize("c", [_case(64, 3, 3), _case(192, 3, 3)], ids=case_id)
def test_three_launches_with_head_and_tail_against_float64(pkg, c, head):
    hold_to_float64(pkg, c, head, 1)


@pytest.mark.parametrize("c", WIDE_CASES, ids=case_id)
def test_256_channels_beyond_the_three_launches(pkg, c):
    """Where dds_depthwise_kernel has no tile (it says so), dds_layer_kernel is held to float64 itself, and the latency kernel to dds_layer_kernel"""
    with pytest.raises(pkg.VitsError, match="dds_depthwise_kernel needs [0-9]+ bytes of LDS"):
        plan_of(pkg, c, UNFUSED, F32, 1)
    hold_to_float64(pkg, c, 0, 0, variant=LAYER)
    if c["layers"] > 3:
        with pytest.raises(pkg.VitsError, match="dds_layer_lat_kernel needs [0-9]+ bytes of LDS"):
            plan_of(pkg, c, LAT, F32, 1)
        return
    for T in lengths_of(plan_of(pkg, c, LAT, F32, 1)):
        same_valid_bits(run(pkg, c, LAT, F32, T, ragged(T))[0], unfused(pkg, c, F32, T, 0, 0, LAYER)[0], ragged(T), "%s T = %d: latency kernel against dds_layer_kernel" % (case_id(c), T))


# ---- hygiene ---------------------------------------------------------------------------------------------------------------------------------------
FAMILIES = [(UNFUSED, F32), (UNFUSED, F16), (LAYER, F32), (LAYER, F16), (LAYER, BF16), (LAT, F32)]


@pytest.mark.parametrize("head,tail", [(0, 0), (1, 1), (2, 1)], ids=["plain", "from1-proj", "conv-proj"])
@pytest.mark.parametrize("variant,arith", FAMILIES, ids=lambda v: None)
@pytest.mark.parametrize("c", [_case(32, 3, 3), _case(192, 3, 3)], ids=case_id)
def test_hygiene(pkg, c, variant, arith, head, tail):
    nt = plan_of(pkg, c, variant, arith, 1, head, tail)["nt"]
    T = nt + 5
    lens = [T, T - 1, 0, T - 3]
    x, z, cond = inputs_of(c, T)
    z[:, 1] = np.nan  # zc = 0: the other latent row is not read
    y, y2 = run(pkg, c, variant, arith, T, lens, head, tail, inputs=(x, z, cond))
    got = y2 if tail else y
    for out in (y, y2) if tail else (y,):
        if out is y and tail and variant == LAT:
            assert (out.view(np.uint32) == NAN_BITS).all(), "with a tail the latency kernel writes no y"
            continue
        for b, n in enumerate(lens):
            assert np.isfinite(out[b, :, :n]).all(), (b, "a NaN staged behind an utterance, or the unnamed latent row, was read")
            assert (out[b, :, n:].view(np.uint32) == NAN_BITS).all(), (b, "a column behind lens[b] was written")
    # every row == its batch-1 call
    for b, n in enumerate(lens):
        if n == 0:
            continue
        one = result_of(run(pkg, c, variant, arith, T, [n], head, tail, bias_rows=BIAS_ROWS[b:b + 1], inputs=(x[b:b + 1], z[b:b + 1], cond[b:b + 1])), tail)
        same_valid_bits(got[b:b + 1], one, [n], "row %d against its batch-1 call" % b)
    # the same bits at a t_stride far larger than t and at one that is no multiple of 4
    for ts in (T + 1003, T + 1 if (T + 1) % 4 else T + 2):
        wide = [np.zeros(a.shape[:2] + (ts,), np.float32) for a in (x, z, cond)]
        for w, a in zip(wide, (x, z, cond)):
            w[:, :, :T] = a
        other = result_of(run(pkg, c, variant, arith, T, lens, head, tail, ts=ts, inputs=wide), tail)
        assert other.shape[2] == ts
        same_valid_bits(other, got, lens, "t_stride %d against t_stride %d" % (ts, T))
        for b, n in enumerate(lens):
            assert (other[b, :, n:].view(np.uint32) == NAN_BITS).all(), (ts, b, "a column behind lens[b] was written")


def test_the_other_latent_row_is_the_one_zc_names(pkg):
    """zc = 1 reads row 1: the same bits as zc = 0 on swapped rows"""
    c, T = _case(64, 3, 3), 21
    x, z, cond = inputs_of(c, T)
    for variant in (UNFUSED, LAYER, LAT):
        a = run(pkg, c, variant, F32, T, ragged(T), head=1, inputs=(x, z, cond), zc=0)[0]
        b = run(pkg, c, variant, F32, T, ragged(T), head=1, inputs=(x, z[:, ::-1].copy(), cond), zc=1)[0]
        same_valid_bits(a, b, ragged(T), "variant %d: zc" % variant)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
# (case, variant, arithmetic, head, tail rows, what the message says)
REFUSALS = [
    (_case(16, 3, 3), LAYER, F32, 0, 0, "no dds_layer_kernel for channels = 16"),
    (_case(16, 3, 3), LAT, F32, 0, 0, "no dds_layer_lat_kernel for channels = 16"),
    (_case(288, 3, 3), LAYER, F32, 0, 0, "no dds_layer_kernel for channels = 288"),
    (_case(288, 3, 3), LAT, F32, 0, 0, "no dds_layer_lat_kernel for channels = 288"),
    (_case(288, 3, 3), LAYER, F16, 0, 0, "no dds_layer_kernel for channels = 288"),
    (_case(64, 2, 2), LAYER, F32, 0, 0, "(k - 1) * dilation is odd"),
    (_case(64, 2, 2), LAT, F32, 0, 0, "(k - 1) * dilation is odd"),
    (_case(192, 3, 3), LAT, F16, 0, 0, "fp32 only"),
    (_case(192, 3, 3), LAT, BF16, 0, 0, "fp32 only"),
    (_case(32, 3, 3), LAT, F32, 1, 47, "exceeds channels"),  # (3 x 16 bins - 1 rows behind 32 channels)
    (_case(256, 3, 5), LAYER, F32, 0, 0, "layer 4 (k = 3, dilation 81): dds_layer_kernel needs"),
    (_case(256, 3, 4), LAT, F32, 0, 0, "layer 3 (k = 3, dilation 27): dds_layer_lat_kernel needs"),
]


def refusal_id(r):
    return "%s-v%d-%s-%s" % (case_id(r[0]), r[1], ARITH_NAME[r[2]], r[5].split()[0].strip("("))


def check_refusal(pkg, r, run_op=False):
    c, variant, arith, head, rows, cause = r
    pkg.op_set_arith(arith)
    try:
        with pytest.raises(pkg.VitsError) as e:
            pkg.op_dds_block_plan(c["H"], c["k"], c["layers"], 20, batch=4, variant=variant, head=head, tail_rows=rows)
        assert cause in str(e.value) and "vits_op_dds_block" in str(e.value), str(e.value)
        if run_op:
            P = D.make_params(c["H"], c["k"], c["layers"], 1, tail_rows=rows)
            x = np.zeros((4, c["H"], 20), np.float32)
            kw = dict(x=x) if head == 0 else dict(z=np.zeros((4, 2, 20), np.float32), cond=x, head_w=P["from1_w"], head_b=P["from1_b"])
            if rows:
                kw.update(tail_w=P["tail_w"], tail_b=P["tail_b"])
            with pytest.raises(pkg.VitsError) as e2:
                pkg.op_dds_block(P["dw_w"], P["dw_b"], P["g1"], P["b1"], P["pw_w"], P["pw_b"], P["g2"], P["b2"], variant=variant, **kw)
            assert str(e2.value) == str(e.value)
    finally:
        pkg.op_set_arith(F32)


@pytest.mark.parametrize("r", REFUSALS, ids=refusal_id)
def test_refusals_name_their_cause(pkg, r):
    check_refusal(pkg, r, run_op=True)


def test_the_lds_limit_comes_from_the_plan_query(pkg):
    """256 channels, k = 3: the first layer count each fused family refuses is the one whose last dilation passes the limit the message states"""
    for variant, first in ((LAYER, 5), (LAT, 4)):
        for layers in range(1, first):
            assert max(plan_of(pkg, _case(256, 3, layers), variant, F32, 1)["lds"]) <= 150 * 1024
        with pytest.raises(pkg.VitsError, match="bytes of LDS, the limit is 153600"):
            plan_of(pkg, _case(256, 3, first), variant, F32, 1)
