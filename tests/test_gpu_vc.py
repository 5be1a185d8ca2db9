"""Voice conversion on the GPU: against transformers taps (tests/golden/make_golden_vc.py), the f16 rounding fixture, flow invertibility,
batch invariance, windowed / device outputs, the speakers' effect, every refusal, and prepare-on-demand weight accounting."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden, rel_err

pytestmark = pytest.mark.gpu

TOL = {"spec": 1e-5, "post_mean": 1e-4, "post_logstd": 1e-4, "z_q": 1e-4, "noise_prior": 0.0, "z_p": 2e-4, "z_flow": 2e-4}


def read(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def vc_full(pkg):
    m = pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL | pkg.SYNTH_SPEAKERS | pkg.SYNTH_POSTERIOR))
    yield m
    m.close()


def pair_key(i, s, t):
    return "p%s_%s_u%d" % ("m1" if s < 0 else s, "m1" if t < 0 else t, i)


@pytest.mark.parametrize("fixture,model,mode", [("vc_tiny_speakers_hf_export_taps.npz", "tiny_speakers_hf_export.ggml", 1),
                                                ("vc_tiny_speakers_hf_export_refmode_taps.npz", "tiny_speakers_hf_export.ggml", 0),
                                                ("vc_tiny_flows3_taps.npz", "vc_tiny_flows3.ggml", 1),
                                                ("vc_full_synth_taps.npz", None, 1)])
def test_conversion_matches_transformers_taps(pkg, vc_full, fixture, model, mode):
    g = golden(fixture)
    dec = int(g["decimate"][0])
    m = vc_full if model is None else pkg.Model(read(model))
    try:
        for i, s, t in g["pairs"].tolist():
            k = pair_key(i, s, t)
            y = g["pcm%d" % i]
            eps = g[k + "_noise_prior"]
            pcm, lengths, frames = m.convert_batch(y, src=s, tgt=t, mode=mode, noise_kind=pkg.NOISE_EXPLICIT, noise_prior=eps[None], collect_taps=True)
            assert frames[0] == y.size // (int(np.prod([8, 8, 2, 2])) if model is None else 8) == eps.shape[1], k
            assert lengths[0] == int(g[k + "_waveform_len"][0]), k
            for tap, tol in TOL.items():
                got = m.tap(tap)
                if tol == 0.0:
                    np.testing.assert_array_equal(got, g[k + "_" + tap].ravel(), err_msg=k)
                else:
                    assert rel_err(got, g[k + "_" + tap]) < tol, (k, tap, rel_err(got, g[k + "_" + tap]))
            assert rel_err(pcm[0][::dec], g[k + "_waveform"]) < 2e-4, k
            assert rel_err(m.tap("waveform")[::dec], g[k + "_waveform"]) < 2e-4, k
    finally:
        if model is not None:
            m.close()


def test_conversion_f16_matches_the_torch_operand_rounding_fixture(pkg):
    g = golden("vc_tiny_synth_arith_f16_taps.npz")
    tol = 5e-3
    with pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_TINY | pkg.SYNTH_SPEAKERS | pkg.SYNTH_POSTERIOR)) as m:
        m.set_arith(pkg.ARITH_F16)
        for i, s, t in g["pairs"].tolist():
            k = pair_key(i, s, t)
            pcm, lengths, _ = m.convert_batch(g["pcm%d" % i], src=s, tgt=t, mode=pkg.MODE_REFERENCE, noise_kind=pkg.NOISE_EXPLICIT,
                                              noise_prior=g[k + "_noise_prior"][None], collect_taps=True)
            assert lengths[0] == int(g[k + "_waveform_len"][0])
            for a, b in ((m.tap("z_p"), g[k + "_z_p"]), (m.tap("z_flow"), g[k + "_z_flow"]), (pcm[0], g[k + "_waveform"])):
                a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
                rms = np.sqrt((b ** 2).mean())
                assert np.abs(a - b).max() / rms < tol and np.sqrt(((a - b) ** 2).mean()) / rms < tol / 4, k


def signals(n_list, seed=5):
    rng = np.random.default_rng(seed)
    out = np.zeros((len(n_list), max(n_list)), np.float32)
    for b, n in enumerate(n_list):
        t = np.arange(n) / 16000.0
        y = np.sin(2 * np.pi * rng.uniform(100, 250) * t) + 0.3 * np.sin(2 * np.pi * rng.uniform(400, 900) * t) + 0.05 * rng.standard_normal(n)
        out[b, :n] = 0.8 * y / np.abs(y).max()
    return out, np.array(n_list, np.int64)


def test_same_speaker_flow_round_trip_returns_z_q(pkg, vc_full):
    pcm, lens = signals([3001])
    vc_full.convert_batch(pcm, lens, src=12, tgt=12, noise_seed=3, collect_taps=True)
    assert rel_err(vc_full.tap("z_flow"), vc_full.tap("z_q")) < 1e-4


@pytest.mark.parametrize("arith", ["f32", "f16"])
def test_mixed_batch_rows_equal_batch_one_calls(pkg, vc_full, arith):
    vc_full.set_arith(pkg.ARITH_F16 if arith == "f16" else pkg.ARITH_F32)
    try:
        pcm, lens = signals([4100, 2311, 5999, 1024], seed=9)
        src, tgt, offs = [3, -1, 77, 5], [50, 8, -1, 5], [7, 1, 4, 2]
        got, lengths, frames = vc_full.convert_batch(pcm, lens, src=src, tgt=tgt, noise_seed=11, noise_seed_offsets=offs)
        for b in range(4):
            one, l1, f1 = vc_full.convert_batch(pcm[b, :lens[b]], src=src[b], tgt=tgt[b], noise_seed=11, noise_seed_offsets=[offs[b]])
            assert l1[0] == lengths[b] and f1[0] == frames[b] == lens[b] // 256
            np.testing.assert_array_equal(one[0], got[b], err_msg="utterance %d" % b)
    finally:
        vc_full.set_arith(pkg.ARITH_F32)


def test_windowed_vocoder_and_device_output_are_bit_identical(pkg, vc_full):
    import ctypes as C
    pcm, lens = signals([7000, 4100], seed=4)
    want, lengths, _ = vc_full.convert_batch(pcm, lens, src=[1, 2], tgt=[60, 61], noise_seed=2)
    chunks = {}
    got, _, _ = vc_full.convert_batch(pcm, lens, src=[1, 2], tgt=[60, 61], noise_seed=2, vocoder_chunk_frames=7,
                                      on_chunk=lambda u, off, x: chunks.setdefault(u, []).append((off, x)) and False)
    for b in range(2):
        np.testing.assert_array_equal(got[b], want[b])
        np.testing.assert_array_equal(np.concatenate([x for _, x in sorted(chunks[b], key=lambda c: c[0])]), want[b])
    # a caller-owned device buffer from the HIP runtime the library is linked against (as test_gpu_edge_and_scale.py does)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    stride = int(lengths.max()) + 64
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), 2 * stride * 4) == 0
    try:
        none, l2, _ = vc_full.convert_batch(pcm, lens, src=[1, 2], tgt=[60, 61], noise_seed=2, out_device=dev.value, out_device_stride=stride,
                                            skip_host_copy=True)
        assert none is None and np.array_equal(l2, lengths)
        host = np.zeros((2, stride), np.float32)
        assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), dev, host.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        for b in range(2):
            np.testing.assert_array_equal(host[b, :lengths[b]], want[b])
    finally:
        hip.hipFree(dev)


def test_target_and_source_speakers_change_the_audio(pkg, vc_full):
    pcm, lens = signals([4000], seed=6)
    a = vc_full.convert_batch(pcm, lens, src=10, tgt=20, noise_seed=1)[0][0]
    b = vc_full.convert_batch(pcm, lens, src=10, tgt=90, noise_seed=1)[0][0]
    c = vc_full.convert_batch(pcm, lens, src=40, tgt=20, noise_seed=1)[0][0]
    rms = np.sqrt((a.astype(np.float64) ** 2).mean())
    assert np.abs(a - b).max() > 1e-2 * rms and np.abs(a - c).max() > 1e-3 * rms


def test_convenience_entry_point_and_explicit_zero_noise(pkg, vc_full):
    pcm, lens = signals([2600], seed=8)
    y = vc_full.convert(pcm[0], 4, 9)
    assert y.size == vc_full.convert_batch(pcm, lens, src=4, tgt=9)[1][0]
    z = np.zeros((1, 192, 2600 // 256), np.float32)
    a = vc_full.convert_batch(pcm, lens, src=4, tgt=9, noise_kind=pkg.NOISE_EXPLICIT, noise_prior=z)[0][0]
    b = vc_full.convert_batch(pcm, lens, src=4, tgt=9, noise_kind=pkg.NOISE_EXPLICIT, noise_prior=z)[0][0]
    np.testing.assert_array_equal(a, b)


def test_refusals_name_the_utterance_and_the_side(pkg, vc_full):
    pcm, lens = signals([3000, 3000])
    cases = [
        (dict(src=[0, 109], tgt=5), ["src_speakers[1]", "source"]),
        (dict(src=5, tgt=[-2, 3]), ["tgt_speakers[0]", "target"]),
        (dict(src=5, tgt=5, fixed_duration=3), ["fixed_duration"]),
        (dict(src=5, tgt=5, frames_only=True), ["frames_only"]),
        (dict(src=5, tgt=5, async_=True), ["async"]),
        (dict(src=5, tgt=5, speaker_ids=[1, 2]), ["src_speakers", "tgt_speakers"]),
    ]
    for kw, words in cases:
        with pytest.raises(pkg.VitsError) as e:
            vc_full.convert_batch(pcm, lens, **kw)
        for w in words:
            assert w in str(e.value), (kw, str(e.value))
    with pytest.raises(pkg.VitsError, match="utterance 1 has 383 samples"):
        vc_full.convert_batch(pcm, np.array([3000, 383], np.int64))  # max(hop 256, pad 384 + 1) = 385
    vc_full.convert_batch(pcm[:, :385], np.array([385, 385], np.int64))  # the minimum itself
    with pytest.raises(pkg.VitsError, match=r"pcm_lengths\[0\]"):
        vc_full.convert_batch(pcm, np.array([3001, 10], np.int64))
    with pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_TINY | pkg.SYNTH_POSTERIOR)) as single:
        with pytest.raises(pkg.VitsError, match=r"src_speakers\[0\].*single speaker"):
            single.convert_batch(pcm, lens, src=0, tgt=-1)
    with pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_TINY)) as bare:
        with pytest.raises(pkg.VitsError, match="no posterior encoder"):
            bare.prepare_conversion()
        with pytest.raises(pkg.VitsError, match="no posterior encoder"):
            bare.convert_batch(pcm, lens)
    # vits_model_set_ggml_tables only changes stage one: accepted, no effect on a conversion
    a = vc_full.convert_batch(pcm, lens, src=1, tgt=2, noise_seed=5)[0]
    vc_full.set_ggml_tables(1)
    try:
        b = vc_full.convert_batch(pcm, lens, src=1, tgt=2, noise_seed=5)[0]
    finally:
        vc_full.set_ggml_tables(0)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def test_bad_n_fft_is_refused(pkg):
    data = bytearray(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_TINY | pkg.SYNTH_POSTERIOR))
    key, val = b"spectrogram_bins", b"9"
    i = data.index(key) + len(key)
    assert data[i:i + 4] == len(val).to_bytes(4, "little") and data[i + 4:i + 5] == val
    data[i + 4:i + 5] = b"7"  # n_fft 12: not a power of two
    with pkg.Model(bytes(data)) as m:
        with pytest.raises(pkg.VitsError, match="power of two"):
            m.prepare_conversion()


def test_busy_and_in_flight_guards(pkg, vc_full):
    pcm, lens = signals([3000])
    ids = pkg.synth_ids(1, 12)
    vc_full.submit_batch(ids)
    try:
        with pytest.raises(pkg.VitsError, match="batches in flight"):
            vc_full.convert_batch(pcm, lens)
    finally:
        vc_full.wait()


def test_weight_bytes_grow_only_when_conversion_is_prepared(pkg):
    with pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL | pkg.SYNTH_SPEAKERS)) as tts:
        base = tts.weight_bytes
    with pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL | pkg.SYNTH_SPEAKERS | pkg.SYNTH_POSTERIOR)) as m:
        assert m.weight_bytes == base
        m.prepare_conversion()
        after = m.weight_bytes
        assert after > base + 4 * 7_000_000  # the posterior encoder's 7.2 M parameters in fp32, its speaker table, the forward-flow packs
        m.prepare_conversion()  # (once)
        assert m.weight_bytes == after
