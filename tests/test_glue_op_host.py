"""CPU side of the operator tests of the spectrogram, sampling, conv_post and resblock-sum kernels (tests/test_gpu_spectrogram_ops.py, tests/test_gpu_glue_ops.py):
the case tables are legal under the engine's geometry rule and reach the edges they name, the references agree with each other and with independent arithmetic, the
float64 spectrogram reproduces every spec tensor of the committed voice-conversion fixtures, every fp32 restatement has an error against float64 that is finite,
not zero and of fp32 size (a bound of 0 would make the 2x rule vacuous), the Python mirror checks its arguments, the library refuses what needs no device to
refuse, and the new symbols are declared and exported."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import glue_ref as G
import spectrogram_ref as SR
import split_ref as R
from conftest import GOLDEN, ROOT

OPS = ("vits_op_spectrogram", "vits_op_prior_sample", "vits_op_posterior_sample", "vits_op_conv_post", "vits_op_resblock_sum")


# ---- spectrogram ------------------------------------------------------------------------------------------------------------------------------------------------
def test_spectrogram_case_table_is_legal_and_reaches_its_edges():
    assert [SR.fpb_of(n) for n in SR.N_FFTS] == [16, 16, 16, 16, 8, 4] and {SR.fpb_of(512), SR.fpb_of(128)} == {16}
    for n_fft in SR.N_FFTS:
        assert len(SR.hops_of(n_fft)) == 5 and {n_fft, 2} <= set(SR.hops_of(n_fft))
        seen_frames, seen_mod = set(), set()
        for hop in SR.hops_of(n_fft):
            assert SR.geometry_ok(n_fft, hop), (n_fft, hop)
            ns = SR.case_lengths(n_fft, hop)
            mn = SR.min_samples(n_fft, hop)
            assert ns[0] == mn == max(hop, (n_fft - hop) // 2 + 1) and all(n >= mn for n in ns) and len(ns) >= SR.BATCH
            fpb = SR.fpb_of(n_fft)
            assert any((n // hop) % fpb == 0 for n in ns) and any((n // hop) % fpb == 1 for n in ns) and any((n // hop) % fpb == fpb - 1 for n in ns), (n_fft, hop)
            assert SR.frame_indices(mn, n_fft, hop).min() >= 0 and SR.frame_indices(mn, n_fft, hop).max() < mn
            seen_frames |= {n // hop for n in ns}
            seen_mod |= {("0" if n % hop == 0 else "1" if n % hop == 1 else "hop-1" if n % hop == hop - 1 else "") for n in ns if hop > 2}
            assert {n % hop for n in ns} >= ({0, 1} if hop > 1 else {0})
        assert set(SR.frame_counts(n_fft)) <= seen_frames, (n_fft, sorted(seen_frames))
        assert {"0", "1", "hop-1"} <= seen_mod
        assert SR.bins_of(n_fft) == (n_fft // 2 + 1, n_fft // 2, 1)
    assert not SR.geometry_ok(48, 8) and not SR.geometry_ok(64, 15) and not SR.geometry_ok(64, 66) and not SR.geometry_ok(4096, 2) and not SR.geometry_ok(8, 2)


def vc_fixture_specs():
    out = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "vc_*_taps.npz"))):
        g = np.load(path)
        for k in g.files:
            m = re.match(r"p(m1|\d+)_(m1|\d+)_u(\d+)_spec$", k)
            if m:
                out.append((os.path.basename(path), k, g["pcm" + m.group(3)], g[k]))
    return out


def test_float64_spectrogram_reproduces_every_fixture_spec_and_the_restatement_follows():
    specs = vc_fixture_specs()
    assert len(specs) >= 15 and {s[3].shape[0] for s in specs} == {9, 513}
    for name, key, y, want in specs:
        n_fft = 2 * (want.shape[0] - 1)
        hop = {16: 8, 1024: 256}[n_fft]
        ref = SR.spectrogram64(y, n_fft, hop)
        assert ref.shape == want.shape == (n_fft // 2 + 1, y.size // hop), (name, key)
        rms = np.sqrt((ref ** 2).mean())
        assert np.abs(want - ref).max() / rms < 1e-5, (name, key)
        assert np.abs(SR.spectrogram32(y, n_fft, hop) - ref).max() / rms < 1e-5, (name, key, "fp32 restatement")


@pytest.mark.parametrize("n_fft", SR.N_FFTS)
def test_spectrogram_restatement_is_within_reach_of_float64_on_every_case(n_fft):
    log2n = n_fft.bit_length() - 1
    for hop in SR.hops_of(n_fft):
        for quiet in (False, True):
            for i, n in enumerate(SR.case_lengths(n_fft, hop)):
                y = SR.signal(n_fft, hop, n, i, quiet)
                ref, chain = SR.spectrogram64(y, n_fft, hop), SR.spectrogram32(y, n_fft, hop)
                assert ref.shape == chain.shape == (n_fft // 2 + 1, n // hop) and np.isfinite(chain).all() and (chain > 0).all()
                rms, _ = R.rms_err(chain, ref)
                # an fp32 FFT loses about sqrt(log2 n) roundings per output: well inside log2 n + 3 of them (window, product, root)
                assert 0 < rms < (log2n + 3) * 2.0 ** -24, (n_fft, hop, quiet, n, rms)
                assert np.array_equal(SR.spectrogram32(y, n_fft, hop, bins=1), chain[:1]) and np.array_equal(SR.spectrogram64(y, n_fft, hop, bins=n_fft // 2), ref[:-1])
                if quiet:
                    floor = np.delete(ref, [0, 1, n_fft // 4, n_fft // 4 + 1, n_fft // 4 + 2], axis=0)[:, 1:-1]  # (edge frames hold a reflected, broken tone)
                    if floor.size and n_fft - hop <= 2:
                        # the noise adds 1e-4 sqrt(3 n_fft / 8) <= 2.8e-3 rms to a bin: the same size as the floor itself
                        assert floor.max() < 2e-2 and floor.min() >= 1e-3 * (1 - 1e-9), (n_fft, hop, floor.max())


def test_spectrogram_tables_and_bit_reversal():
    tw_re, tw_im, win = SR.tables32(16)
    assert tw_re[0] == 1 and tw_im[0] == 0 and tw_im[4] == -1 and abs(tw_re[4]) < 1e-7 and win[0] == 0 and win[8] == 1
    y = np.random.default_rng(1).standard_normal(64).astype(np.float32)
    # hop = n_fft: no pad, a frame is the windowed block itself: the restatement against a plain DFT sum
    got = SR.spectrogram32(y, 16, 16)
    m = np.arange(16)
    for t in range(4):
        X = np.array([(y[16 * t:16 * t + 16].astype(np.float64) * (0.5 - 0.5 * np.cos(2 * np.pi * m / 16)) * np.exp(-2j * np.pi * k * m / 16)).sum() for k in range(9)])
        assert np.allclose(got[:, t], np.sqrt(np.abs(X) ** 2 + 1e-6), rtol=1e-5, atol=1e-6)


# ---- sampling ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_sampling_case_tables_and_the_gather():
    assert set(G.SAMPLE_FRAMES) >= {1, 255, 256, 257} and max(G.SAMPLE_FRAMES) > 512
    assert {c for c in G.SAMPLE_CHANNELS if c < 16} and {c for c in G.SAMPLE_CHANNELS if c % 16} and 192 in G.SAMPLE_CHANNELS and 16 in G.SAMPLE_CHANNELS
    for kind in G.DURATION_KINDS:
        for T, L in ((12, 257), (9, 1), (9, 512), (1, 255), (5, 0)):
            if (kind == "none") != (L == 0):
                continue
            d = G.durations_case(kind, T, L)
            assert d.shape == (T,) and d.sum() == L and (d >= 0).all()
            if kind.startswith("zeros") and T >= 9:
                run = T // 4
                assert (kind not in ("zeros_start", "zeros_everywhere") or not d[:run].any()) and (kind not in ("zeros_end", "zeros_everywhere") or not d[T - run:].any())
                assert kind != "zeros_middle" or not d[T // 2 - run // 2:T // 2 - run // 2 + run].any()
            cum, tl, fr = G.cum_rows([d], T + 3)
            assert (cum[0, T:] == G.SENTINEL).all() and tl[0] == T and fr[0] == max(1, L)
            a = G.token_of_frame(cum[0], T, fr[0])
            brute = np.array([next((i for i in range(T) if cum[0, i] > j), -1) for j in range(fr[0])])
            assert np.array_equal(a, brute)
            if L:
                assert np.array_equal(np.bincount(a, minlength=T), d), "every token holds its duration's frames"
            else:
                assert (a == -1).all()


def test_counter_stream_matches_the_library_and_the_samplers_agree(pkg):
    # the hash: the library's synthetic ids are 1 + (hash3(seed + utt, 3, t) >> 33) % (vocab - 1) at odd t (include/vits_synth_noise.h)
    ids = np.asarray(pkg.synth_ids(3, 64, vocab=38, ids_seed=1234))
    for utt in range(3):
        t = np.arange(64, dtype=np.uint64)
        want = 1 + ((G._hash3(1234 + utt, 3, t) >> np.uint64(33)) % np.uint64(37)).astype(np.int64)
        want[0::2] = 0
        assert np.array_equal(ids[utt], want)
    z = G.counter_normal(7, G.STREAM_NOISE_PRIOR, np.arange(1 << 16))
    assert z.dtype == np.float32 and abs(float(z.mean())) < 0.02 and abs(float(z.std()) - 1) < 0.02 and np.abs(z).max() < 4.9
    assert not np.array_equal(z, G.counter_normal(8, G.STREAM_NOISE_PRIOR, np.arange(1 << 16)))
    draw = G.counter_noise(7, np.array([0, 1], np.int32), 3, [5, 2], 6)
    assert np.array_equal(draw[0, :, :5].ravel(), z[:15]) and np.isnan(draw[0, :, 5:]).all() and np.isnan(draw[1, :, 2:]).all()
    assert np.array_equal(draw[1, :, :2].ravel(), G.counter_normal(8, G.STREAM_NOISE_PRIOR, np.arange(6)))
    rng = np.random.default_rng(2)
    mu, lv, eps = (rng.standard_normal((2, 3, 400)).astype(np.float32) for _ in range(3))
    for scale in (0.667, np.array([0.5, 1.25], np.float32)):
        ref = G.sample64(mu, lv, eps, scale)
        rms, _ = R.rms_err(G.prior32(mu, lv, eps, scale), ref)
        assert 0 < rms < 4 * 2.0 ** -24, rms
    assert np.array_equal(G.prior32(mu, lv, eps, 0.0), mu) and np.array_equal(G.prior32(0 * mu, 0 * lv, eps, 1.0), eps)
    rms, _ = R.rms_err(G.posterior32(mu, lv, eps, 0.5), G.sample64(mu, lv, eps, 0.5))
    assert 0 < rms < 4 * 2.0 ** -24, rms
    assert np.array_equal(G.posterior32(mu, lv, eps, 0.0), mu)


# ---- conv_post and the sum --------------------------------------------------------------------------------------------------------------------------------------
def test_conv_post_case_tables():
    assert {c % 8 for c in G.POST_CIN} >= {0, 1, 7} and max(G.POST_CIN) > 32 and 7 in G.POST_K and len(G.POST_K) == 3
    assert {T for T in G.POST_LENGTHS if T < 4} and {1023, 1024, 1025} <= set(G.POST_LENGTHS) and max(G.POST_LENGTHS) > 2048
    assert {lo % 4 for lo in G.POST_EMIT_LO} == {0, 2} and 1024 in G.POST_EMIT_LO
    assert G.emit_his(100, 4) == [4, 95, 99, 100] and G.emit_his(3, 0) == [0, 2, 3]
    for T in G.POST_LENGTHS:
        assert G.odd_pitch(T) >= T and G.odd_pitch(T) % 4 and G.aligned_pitch(T) >= T and G.aligned_pitch(T) % 4 == 0
    assert all(c % 8 == 0 for c in G.POST16_CIN) and all(c % 8 for c in G.POST16_CIN_FP32_LAYOUT)
    assert sum(G.POST_LENGTHS) + sum(G.POST_RAGGED) >= G.MIN_ELEMS


@pytest.mark.parametrize("arith_name", ("f32", "f16", "bf16"))
def test_conv_post_references_agree(arith_name):
    for cin, k in ((1, 3), (9, 7), (40, 5)):
        lens = [37, 5, 1]
        x, w = G.post_case(cin, k, 37, 3)
        ref, chain = G.post_reference(x, w, 0.01, lens, arith_name)
        assert ref.shape == chain.shape == (sum(lens),) and chain.dtype == np.float32
        # the sums written out: pre[t] = sum_c sum_j w[c][j] a[c][t + j - pad], zero outside the row
        a = G.round16(np.where(x > 0, x, x * np.float32(0.01)), arith_name).astype(np.float64)
        wr = G.round16(w, arith_name).astype(np.float64)
        pad, o = (k - 1) // 2, 0
        for b, n in enumerate(lens):
            for t in range(n):
                s = sum(wr[c, j] * a[b, c, t + j - pad] for c in range(cin) for j in range(k) if 0 <= t + j - pad < n)
                assert abs(ref[o + t] - s) <= 1e-12 * (1 + abs(s)), (cin, k, b, t)
            o += n
        rms, _ = R.rms_err(chain, ref)
        assert rms < np.sqrt(cin * k) * 2.0 ** -24 and (rms > 0 or cin * k < 8), (cin, k, rms)
    assert np.array_equal(G.round16(np.float32([1 + 2.0 ** -11, 1 + 2.0 ** -8 + 2.0 ** -9]), "f16"), np.float32([1, 1 + 2.0 ** -8 + 2.0 ** -9]))
    assert np.array_equal(G.round16(np.float32([1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8]), "bf16"), np.float32([1, 1 + 2.0 ** -6]))
    p = np.float32([0.5, -3.0, 1e-3])
    exact = np.tanh(p.astype(np.float64)).astype(np.float32)  # correctly rounded: half a spacing at most
    assert G.tanh_within(exact, p) <= 0.5 and 0.5 <= G.tanh_within(np.nextafter(exact, np.float32(2)), p) <= 1.5  # ... and one step away, one spacing more


def test_resblock_sum_reference_and_cases():
    assert {T for _, T in G.SUM_CASES} >= {1, 255, 256, 257}
    y = [np.float32([[[1.0, -2.0, 3.0]]]), np.float32([[[0.5, 0.25, -8.0]]]), np.float32([[[1.0, 1.0, 1.0]]])]
    assert np.array_equal(G.sum32(y[0], y[1], None, 2.0, False, False, 0.1), np.float32([[[3.0, -3.5, -10.0]]]))
    assert np.array_equal(G.sum32(y[0], y[1], y[2], 2.0, True, True, 0.5), np.float32([[[1.25, -0.1875, -1.0]]]))


def test_seeded_defects_break_the_rule():
    """one wrong end sample in one row of a pooled case is far outside the 2x rule: the pooling does not hide what the tests are there to find"""
    # spectrogram: the reflection one sample off at the end of ONE utterance of the case (the last frame alone reads it)
    n_fft, hop = 64, 16
    pool = R.EdgePool()
    for i, n in enumerate(SR.case_lengths(n_fft, hop)):
        y = SR.signal(n_fft, hop, n, i, False)
        bad = y.copy()
        if i == 3:
            bad[-2] = y[-3]
        ref, chain = SR.spectrogram64(y, n_fft, hop), SR.spectrogram32(y, n_fft, hop)
        pool.add(SR.spectrogram32(bad, n_fft, hop), ref, chain, np.arange(ref.shape[0]), np.ones(ref.shape[1], bool))
    assert pool.n >= R.MIN_ELEMS and pool.ratio() > 100 * R.FACTOR, pool.ratio()
    # conv_post: the last tap dropped at the last sample of one row of the ragged batch
    lens = list(G.POST_RAGGED)
    x, w = G.post_case(32, 7, max(lens), len(lens))
    ref, chain = G.post_reference(x, w, 0.01, lens)
    got = chain.copy()
    a = np.where(x > 0, x, x * np.float32(0.01))
    end = lens[0] + lens[1] - 1  # row 1's last sample: its tap j = 2 reads the row's own last-but-one input
    got[end] -= np.float32((w[:, 2] * a[1, :, lens[1] - 2]).sum())
    g, c = R.rms_err(got, ref)[0], R.rms_err(chain, ref)[0]
    assert ref.size < R.MIN_ELEMS <= ref.size + sum(G.POST_LENGTHS) and g > 100 * R.FACTOR * c, (g, c)
    # the gather: an off-by-one at a token boundary moves one frame to the neighbouring token
    cum, tl, fr = G.cum_rows([G.durations_case("plain", 12, 257)], 12)
    a = G.token_of_frame(cum[0], 12, 257)
    assert (np.searchsorted(cum[0, :12].astype(np.int64), np.arange(257), side="left") != a).sum() == np.count_nonzero(np.diff(a)) + (a[0] > 0)


# ---- the mirror and the library ---------------------------------------------------------------------------------------------------------------------------------
def test_mirror_checks_its_arguments(pkg):
    z = np.zeros((2, 4, 8), np.float32)
    cum = np.zeros((2, 8), np.int32)
    with pytest.raises(AssertionError):
        pkg.op_spectrogram(np.zeros((1, 2, 64), np.float32), 16, 8)
    with pytest.raises(AssertionError):
        pkg.op_spectrogram(np.zeros((2, 64), np.float32), 16, 8, n_samples=[64])
    with pytest.raises(AssertionError):
        pkg.op_spectrogram(np.zeros(64, np.float32), 16, 0)
    with pytest.raises(AssertionError):
        pkg.op_prior_sample(z, z[:, :3], cum, [8, 8])
    with pytest.raises(AssertionError):
        pkg.op_prior_sample(z, z, cum[:, :7], [8, 8])
    with pytest.raises(AssertionError):
        pkg.op_prior_sample(z, z, cum, [8, 8], noise=np.zeros((2, 4, 9), np.float32))
    with pytest.raises(AssertionError):
        pkg.op_prior_sample(z, z, cum, [8, 8], noise_scales=[1.0])
    with pytest.raises(AssertionError):
        pkg.op_posterior_sample(z, z, [8])
    with pytest.raises(AssertionError):
        pkg.op_posterior_sample(z, z, [8, 8], seed_offsets=[1])
    with pytest.raises(AssertionError):
        pkg.op_conv_post(z, np.zeros((5, 7), np.float32), 0.1)
    with pytest.raises(AssertionError):
        pkg.op_conv_post(z, np.zeros((2, 4, 7), np.float32), 0.1)
    with pytest.raises(AssertionError):
        pkg.op_conv_post(z, np.zeros((4, 7), np.float32), 0.1, emit_hi=[8])
    with pytest.raises(AssertionError):
        pkg.op_resblock_sum(z, z[:1])
    with pytest.raises(AssertionError):
        pkg.op_resblock_sum(z, z, lens=[8])


def test_library_refuses_without_a_device(pkg):
    """geometry and shape refusals come before the first device call"""
    with pytest.raises(pkg.VitsError) as e:
        pkg.op_spectrogram(np.zeros(100, np.float32), 48, 8)
    assert "vits_op_spectrogram" in str(e.value) and "power of two in [16, 2048]" in str(e.value)
    with pytest.raises(pkg.VitsError) as e:
        pkg.op_spectrogram(np.zeros(24, np.float32), 64, 16)
    assert "at least 25 are needed" in str(e.value) and "reflection pad of 24" in str(e.value)
    z = np.zeros((1, 4, 8), np.float32)
    with pytest.raises(pkg.VitsError) as e:
        pkg.op_conv_post(z, np.zeros((4, 4), np.float32), 0.1)
    assert "an odd tap count" in str(e.value)
    with pytest.raises(pkg.VitsError) as e:
        pkg.op_conv_post(z, np.zeros((4, 7), np.float32), 0.1, layout=pkg.CONV_POST_STREAM)
    assert "16-bit arithmetic" in str(e.value)
    with pytest.raises(pkg.VitsError) as e:
        pkg.op_resblock_sum(z, z, in_pitch=7)
    assert "must reach t = 8" in str(e.value)
    with pytest.raises(pkg.VitsError) as e:
        pkg.op_posterior_sample(z, z, [9])
    assert "frames = 9" in str(e.value)


def test_new_symbols_are_declared_exported_and_typed(pkg):
    header = open(os.path.join(ROOT, "include", "vits.h")).read()
    L = pkg.lib()
    for name in OPS:
        assert name in pkg.EXPORTED_SYMBOLS and "VITS_API int " + name + "(" in header and hasattr(L, name) and getattr(L, name).restype == C.c_int32
    assert len(L.vits_op_spectrogram.argtypes) == 9 and len(L.vits_op_prior_sample.argtypes) == 15 and len(L.vits_op_posterior_sample.argtypes) == 12
    assert len(L.vits_op_conv_post.argtypes) == 7 and len(L.vits_op_resblock_sum.argtypes) == 14
    assert [f[0] for f in pkg.ConvPostDesc._fields_] == ["batch", "cin", "k", "t", "x_pitch", "pre_pitch", "slope", "emit_lo", "layout"]
    assert C.sizeof(pkg.ConvPostDesc) == 36
    assert "#define VITS_CONV_POST_FP32_LAYOUT 0" in header and "#define VITS_CONV_POST_STREAM 1" in header and (pkg.CONV_POST_FP32_LAYOUT, pkg.CONV_POST_STREAM) == (0, 1)
    srcs = open(os.path.join(ROOT, "vits.cpp_amd", "csrc", "abi_ops_glue.cpp")).read()
    for launcher in ("launch_spectrogram", "launch_zp", "launch_posterior_sample", "launch_conv_post(", "launch_to_group16", "launch_conv_post16", "launch_rb_sum3_std"):
        assert launcher in srcs, launcher
    assert "__global__" not in srcs, "the operators run the engine's kernels: no second copy"
    for shared in ("stft_geometry(", "stft_tables("):
        assert shared in srcs and shared in open(os.path.join(ROOT, "vits.cpp_amd", "csrc", "engine_convert.cpp")).read(), shared
