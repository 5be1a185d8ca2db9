"""Forced alignment on the device (vits_model_align_batch, align.hip): VITS monotonic alignment search between the text encoder's prior statistics and
z_p of a recording. The search is checked for exact equality against a numpy fp32 restatement run on the GPU's own likelihood matrix, the matrix against
the float64 formula, the whole against transformers fixtures (tests/golden/make_golden_align.py) by a bound that is a theorem, not a measurement."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden, rel_err

pytestmark = pytest.mark.gpu

# max |align_logp - float64 formula on the same call's taps| / RMS(float64) measured on an MI355X over the fixture cases of
# test_logp_matches_the_float64_formula: 3.71e-6 (tiny exporter file, case 2; numpy's fp32 evaluation of the same formula on the same taps: 1.48e-6;
# full-size synthetic model: 9.45e-7). fp32 operand planes, c_t and the K = 2F products accumulated in one k-ordered fp32 chain. The bound is 4 x that.
LOGP_MEASURED = 3.71e-6
LOGP_TOL = 4 * LOGP_MEASURED
ZP_TOL = 2e-4  # test_gpu_vc.py's z_p tolerance against transformers: the floor of align_logp's distance to the fixture's logp64

MODELS = [("align_tiny_speakers_hf_export_taps.npz", "tiny_speakers_hf_export.ggml", 1),
          ("align_tiny_speakers_hf_export_refmode_taps.npz", "tiny_speakers_hf_export.ggml", 0),
          ("align_tiny_flows3_taps.npz", "vc_tiny_flows3.ggml", 1),
          ("align_full_synth_taps.npz", None, 1)]


def read(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def logp_formula(m, ls, z, dt):              # m, ls [F][T]; z [F][L]
    m, ls, z = m.astype(dt), ls.astype(dt), z.astype(dt)
    s = np.exp(-2 * ls)
    c = (-0.5 * np.log(2 * np.pi) - ls).sum(0) + (-0.5 * m * m * s).sum(0)
    return (c[:, None] + s.T @ (-0.5 * z * z) + (m * s).T @ z).astype(dt)      # [T][L]


def mas(lp):
    """VITS maximum_path_each restated; lp [T][L], T <= L, in lp's own precision. Returns (durations, score, path [L])."""
    T, L = lp.shape
    dt = lp.dtype
    NEG = dt.type(-1e9)
    prev_row = np.full(T, NEG, dt)
    down = np.zeros((L, T), bool)
    xs = np.arange(T)
    for y in range(L):
        lo, hi = max(0, T + y - L), min(T - 1, y)
        cur = np.where(xs == y, NEG, prev_row)
        prev = np.concatenate(([dt.type(0) if y == 0 else NEG], prev_row[:-1]))
        down[y] = (xs != 0) & ((xs == y) | (cur < prev))
        row = prev_row.copy()
        row[lo:hi + 1] = (lp[:, y] + np.maximum(prev, cur))[lo:hi + 1]
        prev_row = row
    d = np.zeros(T, np.int32)
    path = np.zeros(L, np.int32)
    i = T - 1
    for y in range(L - 1, -1, -1):
        d[i] += 1
        path[y] = i
        if down[y, i]:
            i -= 1
    return d, prev_row[T - 1], path


def path_score64(lp64, path):
    return float(lp64[path, np.arange(path.size)].sum())


def signals(n_list, seed=5, rate=16000.0):
    rng = np.random.default_rng(seed)
    out = np.zeros((len(n_list), max(n_list)), np.float32)
    for b, n in enumerate(n_list):
        t = np.arange(n) / rate
        y = np.sin(2 * np.pi * rng.uniform(100, 250) * t) + 0.3 * np.sin(2 * np.pi * rng.uniform(400, 900) * t) + 0.05 * rng.standard_normal(n)
        out[b, :n] = 0.8 * y / np.abs(y).max()
    return out, np.array(n_list, np.int64)


def make_ids(B, T, vocab, seed):
    rng = np.random.default_rng(seed)
    ids = np.zeros((B, T), np.int32)
    ids[:, 1::2] = rng.integers(1, vocab, size=ids[:, 1::2].shape)
    return ids


@pytest.fixture(scope="module")
def full(pkg):
    m = pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL | pkg.SYNTH_SPEAKERS | pkg.SYNTH_POSTERIOR))
    yield m
    m.close()


def open_model(pkg, full, name):
    return full if name is None else pkg.Model(read(name))


def check_search_exact(m, B, tl, durations, frames, scores, where):
    """durations, align_path and score of the call equal the numpy fp32 search on the call's own align_logp tap, element for element"""
    for b in range(B):
        T, L = int(tl[b]), int(frames[b])
        lp = m.tap("align_logp", b).reshape(T, L)
        d, sc, path = mas(lp)
        np.testing.assert_array_equal(durations[b, :T], d, err_msg="%s utterance %d" % (where, b))
        assert not durations[b, T:].any(), (where, b)
        np.testing.assert_array_equal(m.tap("align_path", b).astype(np.int32), path, err_msg="%s utterance %d" % (where, b))
        assert np.float32(scores[b]).tobytes() == np.float32(sc).tobytes(), (where, b, scores[b], sc)
        assert durations[b, :T].min() >= 1 and durations[b, :T].sum() == L


# ---- 1. the search is exact ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture,model,mode", MODELS)
def test_search_equals_the_numpy_search_on_its_own_logp(pkg, full, fixture, model, mode):
    m = open_model(pkg, full, model)
    try:
        hop, vocab = m.hop, m.vocab_size
        # ragged batch: T = L (all ones), T = 1, a band one token wide for many frames (T = L - 1), and ordinary utterances
        tl = np.array([23, 1, 40, 17, 9], np.int32)
        fr = np.array([23, 31, 41, 90, 64])
        pcm, lens = signals([int(f * hop + (3 if hop > 3 else 0)) for f in fr], seed=11)
        ids = make_ids(5, int(tl.max()), vocab, 3)
        spk = [0, -1, 2, 1, -1] if m.num_speakers > 1 else -1
        d, frames, sc = m.align_batch(pcm, ids, lens, tl, speakers=spk, mode=mode, collect_taps=True)
        np.testing.assert_array_equal(frames, fr)
        check_search_exact(m, 5, tl, d, frames, sc, fixture)
        np.testing.assert_array_equal(d[0, :23], np.ones(23, np.int32))
        assert d[1, 0] == 31
    finally:
        if model is not None:
            m.close()


@pytest.mark.parametrize("T,L", [(1100, 1300), (2048, 2100), (1025, 700 + 1025)])
def test_search_is_exact_above_1024_tokens_and_with_the_decision_bits_in_the_arena(pkg, T, L):
    """More than one token per lane; (1025, 1725) needs 18 x 1725 64-bit words = 248 KB of decision bits: the arena path"""
    with pkg.Model(read("tiny_speakers_hf_export.ggml")) as m:
        hop = m.hop
        tl = np.array([T, 37], np.int32)
        fr = [L, 50]
        pcm, lens = signals([f * hop for f in fr], seed=T)
        ids = make_ids(2, T, m.vocab_size, T)
        d, frames, sc = m.align_batch(pcm, ids, lens, tl, speakers=[1, 0], collect_taps=True)
        np.testing.assert_array_equal(frames, fr)
        check_search_exact(m, 2, tl, d, frames, sc, "T%d" % T)


# ---- 2. logp is right ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture,model,mode", MODELS)
def test_logp_matches_the_float64_formula(pkg, full, fixture, model, mode):
    g = golden(fixture)
    m = open_model(pkg, full, model)
    try:
        worst = 0.0
        for k, (i, j, s) in enumerate(g["cases"].tolist()):
            y, ids = g["pcm%d" % i], g["ids%d" % j]
            F, T, L = g["c%d_prior_mean" % k].shape[0], ids.size, y.size // m.hop
            eps = np.random.default_rng(k).standard_normal((1, F, L)).astype(np.float32)
            d, frames, sc = m.align_batch(y, ids, speakers=s, noise_scale=1.0, mode=mode, noise_kind=pkg.NOISE_EXPLICIT, noise_prior=eps, collect_taps=True)
            taps = {n: m.tap(n) for n in ("prior_mean", "prior_logvar", "z_p", "z_q", "align_logp")}
            want = logp_formula(taps["prior_mean"].reshape(F, T), taps["prior_logvar"].reshape(F, T), taps["z_p"].reshape(F, L), np.float64)
            err = rel_err(taps["align_logp"], want)
            cpu32 = rel_err(logp_formula(taps["prior_mean"].reshape(F, T), taps["prior_logvar"].reshape(F, T), taps["z_p"].reshape(F, L), np.float32), want)
            print("align_logp vs float64 on its own taps: %s case %d: %.3g (numpy fp32 on the same taps: %.3g)" % (fixture, k, err, cpu32))
            worst = max(worst, err)
            # the call's taps are, bit for bit, those of convert_batch / process_batch on the same inputs, noise and noise_scale = 1
            m.convert_batch(y, src=s, tgt=s, mode=mode, noise_kind=pkg.NOISE_EXPLICIT, noise_prior=eps, collect_taps=True)
            np.testing.assert_array_equal(m.tap("z_p"), taps["z_p"])
            np.testing.assert_array_equal(m.tap("z_q"), taps["z_q"])
            m.process_batch(ids, mode=mode, noise_seed=1, collect_taps=True)
            np.testing.assert_array_equal(m.tap("prior_mean"), taps["prior_mean"])
            np.testing.assert_array_equal(m.tap("prior_logvar"), taps["prior_logvar"])
        print("align_logp worst over %s: %.3g" % (fixture, worst))
        assert worst < LOGP_TOL, worst
    finally:
        if model is not None:
            m.close()


# ---- 3. end to end against transformers ---------------------------------------------------------------------------------------------------------------
def check_against_fixture(m, g, k, mode, tol_rel, where):
    i, j, s = g["cases"][k].tolist()
    y, ids = g["pcm%d" % i], g["ids%d" % j]
    lp64 = g["c%d_logp64" % k]
    T, L = lp64.shape
    d, frames, sc = m.align_batch(y, ids, speakers=s, noise_scale=0.0, mode=mode, collect_taps=True)
    assert frames[0] == L and d.shape == (1, T)
    check_search_exact(m, 1, [T], d, frames, sc, where)
    lp = m.tap("align_logp").reshape(T, L).astype(np.float64)
    e = float(np.abs(lp - lp64).max())
    rel = e / np.sqrt((lp64 ** 2).mean())
    s_star = float(g["c%d_score64" % k][0])
    path = m.tap("align_path").astype(np.int64)
    got = path_score64(lp64, path)
    ulp = float(np.spacing(np.float32(abs(s_star))))
    same = bool(np.array_equal(d[0], g["c%d_durations64" % k]))
    print("%s case %d: e = %.3g (%.3g of RMS), S64* = %.6f, S64(path_gpu) = %.6f, same path as the fixture: %s" % (where, k, e, rel, s_star, got, same))
    assert rel < tol_rel, (where, k, rel)
    assert got >= s_star - 2 * L * e - L * ulp, (where, k, got, s_star, e)


@pytest.mark.parametrize("fixture,model,mode", MODELS)
def test_path_is_within_the_proven_bound_of_the_float64_optimum_of_transformers(pkg, full, fixture, model, mode):
    g = golden(fixture)
    m = open_model(pkg, full, model)
    try:
        for k in range(len(g["cases"])):
            check_against_fixture(m, g, k, mode, max(LOGP_TOL, ZP_TOL), fixture)
            for name in ("prior_mean", "prior_logvar"):
                assert rel_err(m.tap(name), g["c%d_%s" % (k, name)]) < 1e-4
            assert rel_err(m.tap("z_p"), g["c%d_z_p" % k]) < ZP_TOL
    finally:
        if model is not None:
            m.close()


# ---- 4. planted timing at operator level ----------------------------------------------------------------------------------------------------------------
def planted(T, L, F, seed):
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(np.arange(1, L), T - 1, replace=False)) if T > 1 else np.array([], np.int64)
    d = np.diff(np.concatenate(([0], cuts, [L]))).astype(np.int32)
    tok = np.repeat(np.arange(T), d)
    m = rng.standard_normal((F, T)).astype(np.float32)
    ls = (-1 + 0.3 * rng.standard_normal((F, T))).astype(np.float32)
    z = (m[:, tok] + 0.5 * np.exp(ls[:, tok]) * rng.standard_normal((F, L))).astype(np.float32)
    return d, m, ls, z


def test_planted_durations_come_back_exactly(pkg):
    shapes = [(17, 65), (65, 304), (257, 649), (33, 54), (40, 40)]
    F = 192
    cases = [planted(T, L, F, 100 + i) for i, (T, L) in enumerate(shapes)]
    tmax, lmax = max(T for T, _ in shapes), max(L for _, L in shapes)
    m = np.zeros((len(shapes), F, tmax), np.float32)
    ls = np.zeros_like(m)
    z = np.zeros((len(shapes), F, lmax), np.float32)
    for b, ((T, L), (d, mm, ll, zz)) in enumerate(zip(shapes, cases)):
        m[b, :, :T], ls[b, :, :T], z[b, :, :L] = mm, ll, zz
    dur, sc = pkg.op_align(m, ls, z, [T for T, _ in shapes], [L for _, L in shapes])
    for b, ((T, L), (d, mm, ll, zz)) in enumerate(zip(shapes, cases)):
        np.testing.assert_array_equal(dur[b, :T], d, err_msg=str((T, L)))
        assert not dur[b, T:].any()
        # one at a time: the same durations and the same score, bit for bit
        d1, s1 = pkg.op_align(mm[None], ll[None], zz[None])
        np.testing.assert_array_equal(d1[0], d)
        assert s1[0].tobytes() == sc[b].tobytes()
        assert abs(float(sc[b]) - path_score64(logp_formula(mm, ll, zz, np.float64), np.repeat(np.arange(T), d))) < 1e-5 * abs(float(sc[b])) + 1e-2


def test_planted_durations_with_two_tokens_per_lane_and_arena_bits(pkg):
    T, L, F = 1500, 4000, 32
    d, m, ls, z = planted(T, L, F, 7)
    dur, sc = pkg.op_align(m[None], ls[None], z[None])
    np.testing.assert_array_equal(dur[0], d)


# ---- 5. round trip with prosody -------------------------------------------------------------------------------------------------------------------------
def test_alignment_feeds_duration_override_and_matches_the_conversion_length(pkg, full):
    hop = full.hop
    pcm, lens = signals([9301, 5000, 7777], seed=2)
    tl = np.array([19, 7, 12], np.int32)
    ids = make_ids(3, 19, full.vocab_size, 5)
    spk = [3, 77, -1]
    d, frames, sc = full.align_batch(pcm, ids, lens, tl, speakers=spk)
    np.testing.assert_array_equal(frames, lens // hop)
    dout = np.full_like(d, -7)
    out, lengths, fr2 = full.process_batch(ids, tl, speaker_ids=spk, duration_override=d, durations_out=dout, noise_seed=3)
    np.testing.assert_array_equal(fr2, lens // hop)
    for b in range(3):
        np.testing.assert_array_equal(dout[b, :tl[b]], d[b, :tl[b]])
    conv, clen, cfr = full.convert_batch(pcm, lens, src=spk, tgt=spk, noise_seed=3)
    np.testing.assert_array_equal(clen, lengths)
    np.testing.assert_array_equal(cfr, fr2)
    starts, ends = pkg.durations_to_seconds(d[1, :7], full)
    assert starts[0] == 0 and abs(ends[-1] - frames[1] * hop / full.sampling_rate) < 1e-12 and np.all(ends[:-1] == starts[1:])


# ---- 6. invariances -------------------------------------------------------------------------------------------------------------------------------------
def test_rows_of_a_ragged_batch_equal_their_batch_one_calls(pkg, full):
    pcm, lens = signals([9301, 5000, 12000, 2600], seed=8)
    tl = np.array([19, 7, 33, 10], np.int32)
    ids = make_ids(4, 33, full.vocab_size, 9)
    spk, offs = [3, -1, 77, 5], [7, 1, 4, 2]
    d, frames, sc = full.align_batch(pcm, ids, lens, tl, speakers=spk, noise_scale=1.0, noise_seed=11, noise_seed_offsets=offs, collect_taps=True)
    lps = [full.tap("align_logp", b) for b in range(4)]
    for b in range(4):
        d1, f1, s1 = full.align_batch(pcm[b, :lens[b]], ids[b, :tl[b]], speakers=spk[b], noise_scale=1.0, noise_seed=11, noise_seed_offsets=[offs[b]],
                                      collect_taps=True)
        np.testing.assert_array_equal(d1[0], d[b, :tl[b]])
        assert f1[0] == frames[b] and s1[0].tobytes() == sc[b].tobytes()
        np.testing.assert_array_equal(full.tap("align_logp"), lps[b])


def test_posterior_mean_ignores_the_noise_and_scale_one_is_the_conversion_draw(pkg, full):
    pcm, lens = signals([9301], seed=4)
    ids = make_ids(1, 19, full.vocab_size, 2)
    L, F = 9301 // full.hop, 192
    eps = np.random.default_rng(0).standard_normal((1, F, L)).astype(np.float32)
    base = full.align_batch(pcm, ids, speakers=5, noise_scale=0.0, noise_seed=1, collect_taps=True)
    zq0 = full.tap("z_q")
    np.testing.assert_array_equal(zq0, full.tap("post_mean"))
    for kw in (dict(noise_seed=99), dict(noise_kind=pkg.NOISE_EXPLICIT, noise_prior=eps), dict(noise_kind=pkg.NOISE_REFERENCE)):
        got = full.align_batch(pcm, ids, speakers=5, noise_scale=0.0, collect_taps=True, **kw)
        for a, b in zip(base, got):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(full.tap("z_q"), zq0)
    full.align_batch(pcm, ids, speakers=5, noise_scale=1.0, noise_kind=pkg.NOISE_EXPLICIT, noise_prior=eps, collect_taps=True)
    zq1 = full.tap("z_q")
    full.convert_batch(pcm, src=5, tgt=5, noise_kind=pkg.NOISE_EXPLICIT, noise_prior=eps, collect_taps=True)
    np.testing.assert_array_equal(full.tap("z_q"), zq1)
    assert not np.array_equal(zq1, zq0)


@pytest.mark.parametrize("arith", ["F16", "BF16", "F32_SPLIT"])
def test_sixteen_bit_and_split_arithmetic_keep_the_search_exact(pkg, full, arith):
    g = golden("align_full_synth_taps.npz")
    full.set_arith(getattr(pkg, "ARITH_" + arith))
    try:
        pcm, lens = signals([9301, 5000], seed=8)
        tl = np.array([19, 7], np.int32)
        ids = make_ids(2, 19, full.vocab_size, 9)
        d, frames, sc = full.align_batch(pcm, ids, lens, tl, speakers=[3, -1], collect_taps=True)
        check_search_exact(full, 2, tl, d, frames, sc, arith)
        # the inequality of the end-to-end test with this call's own e (z_p carries the mode's rounding: 5e-3 of RMS is test_gpu_vc.py's f16 tolerance;
        # bf16 operands have 8 bits less: 4e-2)
        for k in range(len(g["cases"])):
            check_against_fixture(full, g, k, 1, 4e-2 if arith == "BF16" else 5e-3, arith)
    finally:
        full.set_arith(pkg.ARITH_F32)


def test_speakers_change_the_result_and_minus_one_equals_the_speakerless_file(pkg):
    """speaker -1 on the speaker file is, bit for bit, the same file written as a single-speaker model (num_speakers = 1, no embed_speaker)"""
    from test_speakers import read_file, write_file
    data = read("tiny_speakers_hf_export.ggml")
    with pkg.Model(data) as m:
        hop = m.hop
        pcm, lens = signals([90 * hop, 64 * hop], seed=6)
        tl = np.array([30, 17], np.int32)
        ids = make_ids(2, 30, m.vocab_size, 1)
        none = m.align_batch(pcm, ids, lens, tl, speakers=-1, collect_taps=True)
        lp_none = [m.tap("align_logp", b) for b in range(2)]
        m.align_batch(pcm, ids, lens, tl, speakers=[2, 1], collect_taps=True)
        assert not np.array_equal(m.tap("align_logp", 0), lp_none[0]) and not np.array_equal(m.tap("align_logp", 1), lp_none[1])
    v, h, c, t = read_file(data)
    c = [(k, b"1" if k == b"num_speakers" else val) for k, val in c]
    with pkg.Model(write_file(v, h, c, [x for x in t if x[0] != "embed_speaker.weight"])) as m:
        assert m.num_speakers == 1
        got = m.align_batch(pcm, ids, lens, tl, collect_taps=True)
        for a, b in zip(none, got):
            np.testing.assert_array_equal(a, b)
        for b in range(2):
            np.testing.assert_array_equal(m.tap("align_logp", b), lp_none[b])


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_leave_the_handle_usable(pkg, full, tiny_bytes):
    pcm, lens = signals([5000], seed=1)
    ids = make_ids(1, 7, full.vocab_size, 1)
    want = full.align_batch(pcm, ids, speakers=3)
    cases = [(dict(fixed_duration=2), "fixed_duration"), (dict(frames_only=True), "frames_only"), (dict(async_=True), "async"),
             (dict(out_device=1 << 20), "out_device"), (dict(skip_host_copy=True), "skip_host_copy"), (dict(vocoder_chunk_frames=8), "vocoder_chunk_frames"),
             (dict(on_chunk=lambda *a: 0), "on_chunk"), (dict(speaker_ids=[1]), "speaker_ids"), (dict(speaking_rate=[1.0]), "speaking_rates"),
             (dict(noise_scales=[0.5]), "noise_scales"), (dict(noise_scale_duration=[0.5]), "noise_scale_durations"),
             (dict(duration_override=np.ones(7, np.int32)), "duration_override"), (dict(durations_out=np.zeros(7, np.int32)), "durations_out"),
             (dict(noise_scale=float("nan")), "noise_scale"), (dict(noise_scale=10.5), "noise_scale"), (dict(noise_scale=-0.1), "noise_scale"),
             (dict(speakers=109), "outside [-1, 109)"), (dict(speakers=-2), "outside [-1, 109)")]
    for kw, msg in cases:
        args = dict(speakers=3)
        args.update(kw)
        with pytest.raises(pkg.VitsError, match=msg.replace("[", r"\[").replace(")", r"\)")):
            full.align_batch(pcm, ids, **args)
        got = full.align_batch(pcm, ids, speakers=3)
        for a, b in zip(want, got):
            np.testing.assert_array_equal(a, b)
    # more tokens than frames: the message names the utterance, its tokens and its frames
    ids2 = make_ids(2, 25, full.vocab_size, 2)
    pcm2, lens2 = signals([9301, 5000], seed=1)
    with pytest.raises(pkg.VitsError, match=r"utterance 1 has 25 tokens but only 19 frames"):
        full.align_batch(pcm2, ids2, lens2, [25, 25])
    # batches in flight
    full.submit_batch(ids, noise_seed=1)
    with pytest.raises(pkg.VitsError, match="batches in flight"):
        full.align_batch(pcm, ids, speakers=3)
    full.wait()
    got = full.align_batch(pcm, ids, speakers=3)
    for a, b in zip(want, got):
        np.testing.assert_array_equal(a, b)
    # a model file without a posterior encoder
    with pkg.Model(tiny_bytes) as m:
        with pytest.raises(pkg.VitsError, match="no posterior encoder"):
            m.align_batch(np.zeros(4000, np.float32), make_ids(1, 5, m.vocab_size, 1))
        m.process_batch(make_ids(1, 5, m.vocab_size, 1))


def test_weight_bytes_grow_only_when_the_first_alignment_prepares_the_posterior(pkg):
    data = pkg.synth_model_bytes(0x5EED, pkg.SYNTH_TINY | pkg.SYNTH_SPEAKERS | pkg.SYNTH_POSTERIOR)
    with pkg.Model(data) as m:
        ids = make_ids(1, 6, m.vocab_size, 1)
        m.process_batch(ids)
        w0 = m.weight_bytes  # (a first small call has made the latency kernels' copy of the TTS layers)
        m.process_batch(ids)
        assert m.weight_bytes == w0
        pcm, _ = signals([40 * m.hop], seed=1)
        with pytest.raises(pkg.VitsError):
            m.align_batch(pcm, ids, fixed_duration=1)
        assert m.weight_bytes == w0
        m.align_batch(pcm, ids)
        w1 = m.weight_bytes
        assert w1 > w0
        m.align_batch(pcm, ids)
        m.convert_batch(pcm)
        assert m.weight_bytes == w1


def test_align_from_text_tokenizes_and_returns_the_posterior_mean_alignment(pkg):
    with pkg.Model(read("tiny_speakers_hf_export.ggml")) as m:
        pcm, _ = signals([80 * m.hop], seed=3)
        ids, d = m.align(pcm[0], "hello there", speaker=1)
        np.testing.assert_array_equal(ids, m.tokenize("hello there"))
        want, frames, _ = m.align_batch(pcm, ids, speakers=1)
        np.testing.assert_array_equal(d, want[0])
        assert d.sum() == 80 and d.min() >= 1
