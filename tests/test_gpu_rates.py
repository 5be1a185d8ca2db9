"""Any sample rate through the engine (vits_model_set_rates, resample.hip): the delivered PCM is the operator's resampling of the model-rate waveform, bit
for bit, through every way a call can deliver it (batch rows, the pipeline, a device buffer, async, every arithmetic, streaming chunks); recordings at
another rate enter conversion and alignment as the operator's resampling of them; nothing changes when no rate is asked for; the refusals."""
import ctypes as C
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LENS = np.array([5, 12, 31], np.int32)
OUT_RATES = (8000, 24000, 22050, 44100)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def ids(pkg):
    return pkg.synth_ids(3, 31)


@pytest.fixture(scope="module")
def tiny(pkg, tiny_bytes):
    with pkg.Model(tiny_bytes) as m:
        assert m.sampling_rate == 16000 and m.hop == 8
        yield m


@pytest.fixture(scope="module")
def plain(tiny, ids):
    """the call without rates: (pcm, lengths, frames, durations)"""
    tiny.set_rates(0, 0)
    d = np.zeros(ids.shape, np.int32)
    pcm, lengths, frames = tiny.process_batch(ids, id_lengths=LENS, noise_seed=7, durations_out=d)
    return pcm, lengths, frames, d


@pytest.fixture()
def model(pkg, tiny):
    """the shared handle, back at the model's rate and fp32 afterwards"""
    yield tiny
    tiny.set_arith(pkg.ARITH_F32)
    tiny.set_rates(0, 0)


def op(pkg, x, fi, fo):
    y, n = pkg.resample(x, fi, fo)
    return y[0, :n[0]]


@pytest.mark.parametrize("rate", OUT_RATES)
def test_delivered_pcm_is_the_resampled_waveform(pkg, model, ids, plain, rate):
    model.set_rates(output_rate=rate)
    assert model.rates == (0, rate)
    d = np.zeros(ids.shape, np.int32)
    pcm, lengths, frames = model.process_batch(ids, id_lengths=LENS, noise_seed=7, durations_out=d, collect_taps=True)
    assert np.array_equal(frames, plain[2]) and np.array_equal(d, plain[3])
    for b in range(3):
        wave = model.tap("waveform", b).ravel()
        assert same(wave, plain[0][b])  # (the model-rate waveform is what it was)
        want = op(pkg, wave, 16000, rate)
        assert lengths[b] == want.size == pkg.resample_length(16000, rate, wave.size)
        assert same(pcm[b], want), (rate, b)
        assert same(model.tap("waveform_out", b).ravel(), want)
    # frames_only reports the lengths the full call delivers
    _, l2, f2 = model.process_batch(ids, id_lengths=LENS, noise_seed=7, frames_only=True)
    assert np.array_equal(l2, lengths) and np.array_equal(f2, frames)


def test_rows_pipeline_and_device_output_are_the_same_bits(pkg, model, ids, plain):
    model.set_rates(output_rate=44100)
    pcm, lengths, frames = model.process_batch(ids, id_lengths=LENS, noise_seed=7)
    # a row of the ragged batch equals its batch-1 call
    for b in range(3):
        one, l1, _ = model.process_batch(ids[b:b + 1, :LENS[b]], noise_seed=7, noise_seed_offsets=np.array([b], np.int32))
        assert l1[0] == lengths[b] and same(one[0], pcm[b]), b
    # submit / wait
    model.submit_batch(ids, id_lengths=LENS, noise_seed=7)
    model.submit_batch(ids, id_lengths=LENS, noise_seed=7, vocoder_chunk_frames=13)
    for _ in range(2):
        got, l2, f2 = model.wait()
        assert np.array_equal(l2, lengths) and np.array_equal(f2, frames) and all(same(got[b], pcm[b]) for b in range(3))
    # a caller-owned device buffer, without a host copy
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    cap = int(lengths.max()) + 3
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), 3 * cap * 4) == 0
    try:
        none, l3, _ = model.process_batch(ids, id_lengths=LENS, noise_seed=7, out_device=dev.value, out_device_stride=cap, skip_host_copy=True)
        got = np.zeros((3, cap), np.float32)
        assert hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), dev, got.nbytes, 2) == 0
        assert none is None and np.array_equal(l3, lengths) and all(same(got[b, :lengths[b]], pcm[b]) for b in range(3))
        # the stride is checked against the longest DELIVERED utterance (the model-rate waveform would fit)
        assert int(plain[1].max()) < int(lengths.max()) - 1
        with pytest.raises(pkg.VitsError, match="out_device_stride is smaller than the longest utterance"):
            model.process_batch(ids, id_lengths=LENS, noise_seed=7, out_device=dev.value, out_device_stride=int(lengths.max()) - 1, skip_host_copy=True)
        # async with fixed_duration: one more kernel on the stream, no host read
        sync_pcm, l4, _ = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=2)
        assert hip.hipMemcpy(dev, np.zeros((3, cap), np.float32).ctypes.data_as(C.c_void_p), got.nbytes, 1) == 0
        none, l5, _ = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=2, out_device=dev.value, out_device_stride=cap, skip_host_copy=True,
                                          async_=True)
        model.sync()
        assert hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), dev, got.nbytes, 2) == 0
        assert np.array_equal(l4, l5) and all(same(got[b, :l4[b]], sync_pcm[b]) for b in range(3))
    finally:
        hip.hipFree(dev)


@pytest.mark.parametrize("arith", ("ARITH_F16", "ARITH_BF16", "ARITH_F32_SPLIT"))
def test_every_arithmetic_delivers_the_resampling_of_its_own_waveform(pkg, model, ids, arith):
    model.set_arith(getattr(pkg, arith))
    model.set_rates(output_rate=22050)
    pcm, lengths, _ = model.process_batch(ids, id_lengths=LENS, noise_seed=7, collect_taps=True)
    for b in range(3):
        assert same(pcm[b], op(pkg, model.tap("waveform", b).ravel(), 16000, 22050)), (arith, b)


@pytest.mark.parametrize("rate", (8000, 44100))
@pytest.mark.parametrize("window", (8, 13))
def test_streamed_chunks_tile_the_resampled_utterance(pkg, model, ids, rate, window):
    model.set_rates(output_rate=rate)
    whole, lengths, frames = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=3)
    assert frames.max() > 40
    chunks = {}
    pcm, l2, _ = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=3, vocoder_chunk_frames=window,
                                     on_chunk=lambda u, off, x: chunks.setdefault(u, []).append((off, x)) and False)
    assert np.array_equal(l2, lengths)
    starved = 0
    for b in range(3):
        pos = 0
        for off, x in chunks[b]:  # in order, no empty call, no gap, no overlap
            assert off == pos and x.size > 0, (b, off, pos)
            pos += x.size
        assert pos == lengths[b]
        assert same(np.concatenate([x for _, x in chunks[b]]), whole[b]) and same(pcm[b], whole[b]), b
        windows = -(-int(frames[b]) // window)
        assert len(chunks[b]) <= windows
        starved += len(chunks[b]) < windows
    if rate == 8000 and window == 8:
        # the filter's half width (70 samples at 16 kHz) exceeds the first window's 64 final samples: that window delivers nothing
        assert starved > 0
    with pytest.raises(pkg.VitsError, match="aborted by the on_chunk callback"):
        model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=3, vocoder_chunk_frames=window, on_chunk=lambda u, off, x: True)
    again, _, _ = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=3)
    assert all(same(again[b], whole[b]) for b in range(3))


@pytest.fixture(scope="module")
def vc_tiny(pkg):
    with pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_TINY | pkg.SYNTH_POSTERIOR)) as m:
        assert m.sampling_rate == 16000 and m.hop == 8
        yield m


def recordings(rate, seed=5):
    rng = np.random.default_rng(seed)
    lens = np.array([rate // 14, rate // 25 + 3], np.int64)
    x = np.full((2, int(lens.max()) + 2), np.nan, np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = 0.3 * rng.standard_normal(n).astype(np.float32)
    return x, lens


@pytest.mark.parametrize("rate", (44100, 8000))
def test_recordings_at_another_rate_enter_as_their_resampling(pkg, vc_tiny, rate):
    m = vc_tiny
    x, lens = recordings(rate)
    y, n = pkg.resample(x, rate, 16000, lens)
    tok = pkg.synth_ids(2, 9)
    try:
        m.set_rates(0, 0)
        want = m.convert_batch(y, n, noise_seed=3)
        want_al = m.align_batch(y, tok, lengths=n, noise_scale=1.0, noise_seed=3)
        m.set_rates(input_rate=rate)
        got = m.convert_batch(x, lens, noise_seed=3, collect_taps=True)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and np.array_equal(got[2], n // 8)
        for b in range(2):
            assert same(got[0][b], want[0][b]), (rate, b)
            assert same(m.tap("pcm_model", b).ravel(), y[b, :n[b]])
        got_al = m.align_batch(x, tok, lengths=lens, noise_scale=1.0, noise_seed=3, collect_taps=True)
        assert np.array_equal(got_al[0], want_al[0]) and np.array_equal(got_al[1], want_al[1]) and same(got_al[2], want_al[2])
        assert same(m.tap("pcm_model", 1).ravel(), y[1, :n[1]])
    finally:
        m.set_rates(0, 0)


def test_short_recordings_and_the_round_trip(pkg, vc_tiny):
    m = vc_tiny
    try:
        m.set_rates(input_rate=44100)
        # 19 samples at 44.1 kHz are 7 at 16 kHz: below one hop of 8
        with pytest.raises(pkg.VitsError, match=r"19 samples at 44100 Hz = 7 at the model's 16000 Hz"):
            m.convert_batch(np.zeros(19, np.float32))
        with pytest.raises(pkg.VitsError, match=r"19 samples at 44100 Hz = 7 at the model's 16000 Hz"):
            m.align_batch(np.zeros(19, np.float32), np.array([1], np.int32))
        # both kernels in one call: 44.1 kHz in, 44.1 kHz out
        m.set_rates(44100, 44100)
        assert m.rates == (44100, 44100)
        x, lens = recordings(44100)
        pcm, lengths, frames = m.convert_batch(x, lens, noise_seed=3, collect_taps=True)
        for b in range(2):
            n_model = pkg.resample_length(44100, 16000, int(lens[b]))
            assert frames[b] == n_model // 8
            wave = m.tap("waveform", b).ravel()
            assert lengths[b] == pkg.resample_length(16000, 44100, wave.size) and wave.size >= frames[b] * 8
            y, _ = pkg.resample(wave, 16000, 44100)
            assert same(pcm[b], y[0, :lengths[b]])
    finally:
        m.set_rates(0, 0)


def test_nothing_changes_when_nothing_is_asked_for(pkg, tiny_bytes, ids, plain):
    with pkg.Model(tiny_bytes) as m:
        m.process_batch(ids, id_lengths=LENS, noise_seed=7)  # (the first small call makes the latency kernels' weight copy: not the rates' doing)
        w0 = m.weight_bytes
        for rates in ((0, 0), (16000, 16000)):
            m.set_rates(*rates)
            assert m.rates == (0, 0)  # (the model's own rate is stored as 0)
            m.prof_enable(True)
            m.prof_reset()
            pcm, lengths, _ = m.process_batch(ids, id_lengths=LENS, noise_seed=7)
            assert "resample_" not in json.dumps(m.prof_report())
            m.prof_enable(False)
            assert np.array_equal(lengths, plain[1]) and all(same(pcm[b], plain[0][b]) for b in range(3))
            assert m.weight_bytes == w0
        # a rate costs its table, at its first use and once
        m.set_rates(output_rate=8000)
        assert m.weight_bytes == w0
        m.prof_enable(True)
        m.prof_reset()
        m.process_batch(ids, id_lengths=LENS, noise_seed=7)
        assert "resample_out" in json.dumps(m.prof_report())
        m.prof_enable(False)
        L, _, K = pkg.resample_plan(16000, 8000)
        assert m.weight_bytes == w0 + 4 * L * K
        m.process_batch(ids, id_lengths=LENS, noise_seed=7)
        assert m.weight_bytes == w0 + 4 * L * K


def test_refusals_leave_the_rates_as_they_were(pkg, model, ids):
    model.set_rates(0, 24000)
    for bad in ((3999, 24000), (0, 192001), (16000, 44101), (-1, 0)):
        with pytest.raises(pkg.VitsError, match="vits_model_set_rates"):
            model.set_rates(*bad)
        assert model.rates == (0, 24000)
    with pytest.raises(pkg.VitsError, match="L = 44101"):
        model.set_rates(0, 44101)
    # with a batch in flight
    model.submit_batch(ids, id_lengths=LENS, noise_seed=7)
    with pytest.raises(pkg.VitsError, match="batches in flight"):
        model.set_rates(0, 8000)
    model.wait()
    assert model.rates == (0, 24000)
    # from inside on_chunk
    seen = []

    def sink(u, off, x):
        try:
            model.set_rates(0, 8000)
        except pkg.VitsError as e:
            seen.append(str(e))
        return False

    model.process_batch(ids, id_lengths=LENS, noise_seed=7, vocoder_chunk_frames=8, on_chunk=sink)
    assert seen and all("model busy" in s for s in seen)
    assert model.rates == (0, 24000)
