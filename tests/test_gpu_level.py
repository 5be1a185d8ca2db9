"""A stated level through the engine (vits_model_set_level, loudness.hip): what a call reports and delivers is the operator's levelling (vits_op_level) of
the model-rate waveform, bit for bit, through every way a call can deliver it (batch rows, the pipeline, a device buffer, async, vocoder windows, 16-bit
arithmetic, streaming chunks, voice conversion, another output rate); nothing changes when no level is set; the refusals."""
import ctypes as C
import json

import numpy as np
import pytest

import loudness_ref as R

pytestmark = pytest.mark.gpu

LENS = np.array([5, 12, 31], np.int32)  # at fixed_duration = 60 and hop 8: 0.15 s, 0.36 s (both unmeasurable) and 0.93 s (six blocks)
KINDS = (("LEVEL_MEASURE", 0.0, 0.0), ("LEVEL_GAIN", -3.0, 0.0), ("LEVEL_PEAK", -1.0, 0.0), ("LEVEL_LOUDNESS", -23.0, -1.0), ("LEVEL_LOUDNESS", -10.0, -6.0))


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
    """the calls without a level, at fixed_duration 60 and 200: (pcm, lengths, frames, durations)"""
    tiny.set_level(0)
    out = {}
    for fd in (60, 200):
        d = np.zeros(ids.shape, np.int32)
        pcm, lengths, frames = tiny.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=fd, durations_out=d)
        assert tiny.last_levels() is None
        out[fd] = (pcm, lengths, frames, d)
    return out


@pytest.fixture()
def model(pkg, tiny):
    """the shared handle, without a level, at the model's rate and fp32 afterwards"""
    yield tiny
    tiny.set_arith(pkg.ARITH_F32)
    tiny.set_rates(0, 0)
    tiny.set_level(pkg.LEVEL_NONE)


def op(pkg, wave, kind, value, ceiling):
    """the operator on one waveform: (y [N], levels [4])"""
    y, levels = pkg.level(wave, 16000, kind, value, ceiling)
    return y[0, :wave.size], levels[0]


@pytest.mark.parametrize("fd", (60, 200))
@pytest.mark.parametrize("kind,value,ceiling", KINDS)
def test_a_call_reports_and_delivers_the_operators_levelling(pkg, model, ids, plain, kind, value, ceiling, fd):
    k = getattr(pkg, kind)
    model.set_level(k, value, ceiling)
    assert model.level == (k, np.float32(value) if k != pkg.LEVEL_MEASURE else 0.0, np.float32(ceiling) if k == pkg.LEVEL_LOUDNESS else 0.0)
    d = np.zeros(ids.shape, np.int32)
    pcm, lengths, frames = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=fd, durations_out=d, collect_taps=True)
    levels = model.last_levels()
    p = plain[fd]
    assert levels.shape == (3, 4)
    assert np.array_equal(lengths, p[1]) and np.array_equal(frames, p[2]) and np.array_equal(d, p[3])
    for b in range(3):
        wave = model.tap("waveform", b).ravel()
        assert same(wave, p[0][b])  # (the model-rate waveform is what it was)
        y, row = op(pkg, wave, k, value, ceiling)
        assert same(levels[b], row), (kind, b)
        assert same(pcm[b], y), (kind, b)
        assert same(model.tap("waveform_level", b).ravel(), y)
        assert same(y, wave * levels[b, 2])
        if k == pkg.LEVEL_MEASURE:
            assert levels[b, 2] == 1.0 and same(pcm[b], wave)
    # what the rows say, against the restatement
    for b in range(3):
        L, P, nb = R.loudness(p[0][b], 16000)
        assert levels[b, 3] == nb and levels[b, 1] == np.float32(P)
        assert (abs(float(levels[b, 0]) - L) <= 0.01) if nb else (levels[b, 0] == -np.inf)
    if fd == 60:
        assert [int(v) for v in levels[:, 3]] == [0, 0, 6]
        if k == pkg.LEVEL_LOUDNESS:
            assert levels[0, 2] == levels[1, 2] == 1.0  # unmeasurable: left as they are
    else:
        assert (levels[:, 3] > 0).all()


def test_levelling_comes_before_the_resampler(pkg, model, ids, plain):
    model.set_level(pkg.LEVEL_LOUDNESS, -20.0, -3.0)
    model.set_rates(output_rate=44100)
    pcm, lengths, _ = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=60, collect_taps=True)
    levels = model.last_levels()
    for b in range(3):
        wave = model.tap("waveform", b).ravel()
        assert same(wave, plain[60][0][b])
        y, row = op(pkg, wave, pkg.LEVEL_LOUDNESS, -20.0, -3.0)
        assert same(levels[b], row) and same(model.tap("waveform_level", b).ravel(), y)
        out, n = pkg.resample(y, 16000, 44100)
        assert lengths[b] == n[0] and same(pcm[b], out[0, :n[0]]), b
        assert same(model.tap("waveform_out", b).ravel(), pcm[b])


@pytest.mark.parametrize("kind,value,ceiling", (("LEVEL_MEASURE", 0.0, 0.0), ("LEVEL_PEAK", -1.0, 0.0), ("LEVEL_LOUDNESS", -23.0, -1.0)))
def test_rows_pipeline_windows_and_device_output_are_the_same_bits(pkg, model, ids, plain, kind, value, ceiling):
    k = getattr(pkg, kind)
    model.set_level(k, value, ceiling)
    pcm, lengths, frames = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=60)
    levels = model.last_levels()
    # (the anchor of everything below: the rows are the operator's on the plain call's waveform, and MEASURE delivers that waveform)
    for b in range(3):
        y, row = op(pkg, plain[60][0][b], k, value, ceiling)
        assert same(levels[b], row) and same(pcm[b], y), (kind, b)
        assert k != pkg.LEVEL_MEASURE or same(pcm[b], plain[60][0][b])
    # a row of the ragged batch equals its batch-1 call
    for b in range(3):
        one, l1, _ = model.process_batch(ids[b:b + 1, :LENS[b]], noise_seed=7, fixed_duration=60, noise_seed_offsets=np.array([b], np.int32))
        assert l1[0] == lengths[b] and same(one[0], pcm[b]) and same(model.last_levels()[0], levels[b]), b
    # vocoder windows without a sink: levelling runs behind the last window
    got, l2, _ = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=60, vocoder_chunk_frames=13)
    assert np.array_equal(l2, lengths) and all(same(got[b], pcm[b]) for b in range(3)) and same(model.last_levels(), levels)
    # submit / wait: the levels of the batch that wait returned
    model.submit_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=60)
    model.submit_batch(ids[:2], id_lengths=LENS[:2], noise_seed=7, fixed_duration=60, vocoder_chunk_frames=13)
    got, l2, f2 = model.wait()
    assert np.array_equal(l2, lengths) and np.array_equal(f2, frames) and all(same(got[b], pcm[b]) for b in range(3))
    assert same(model.last_levels(), levels)
    got, l2, _ = model.wait()
    assert all(same(got[b], pcm[b]) for b in range(2)) and same(model.last_levels(), levels[:2])
    # a caller-owned device buffer without a host copy, then the same asynchronously
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    cap = int(lengths.max()) + 3
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), 3 * cap * 4) == 0
    try:
        for async_ in (False, True):
            assert hip.hipMemcpy(dev, np.zeros((3, cap), np.float32).ctypes.data_as(C.c_void_p), 3 * cap * 4, 1) == 0
            # (another waveform through the call's own buffers first: a measurement that read them instead of what this call wrote would show)
            model.process_batch(ids[::-1].copy(), id_lengths=LENS[::-1].copy(), noise_seed=11, fixed_duration=60)
            none, l3, _ = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=60, out_device=dev.value, out_device_stride=cap,
                                              skip_host_copy=True, async_=async_)
            if async_:
                model.sync()
            got = np.zeros((3, cap), np.float32)
            assert hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), dev, got.nbytes, 2) == 0
            assert none is None and np.array_equal(l3, lengths) and all(same(got[b, :lengths[b]], pcm[b]) for b in range(3)), async_
            assert not got[0, lengths[0]:].any()  # nothing written behind an utterance
            assert same(model.last_levels(), levels), async_
    finally:
        hip.hipFree(dev)


def test_a_batch_split_inside_the_call_reports_every_row(pkg, tiny_bytes, ids, monkeypatch):
    """vits_model_process_batch runs a large batch as two pipelined parts (VITS_SPLIT_MIN_BATCH): the rows of both parts, side by side"""
    out = {}
    for split in ("0", "2"):
        monkeypatch.setenv("VITS_SPLIT_MIN_BATCH", split)
        with pkg.Model(tiny_bytes) as m:
            m.set_level(pkg.LEVEL_LOUDNESS, -23.0, -1.0)
            pcm, lengths, _ = m.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=200)
            out[split] = (pcm, lengths, m.last_levels())
    assert np.array_equal(out["0"][1], out["2"][1]) and same(out["0"][2], out["2"][2])
    assert out["2"][2].shape == (3, 4) and (out["2"][2][:, 3] > 0).all()
    assert all(same(out["0"][0][b], out["2"][0][b]) for b in range(3))


def test_f16_arithmetic_levels_its_own_waveform(pkg, model, ids):
    model.set_arith(pkg.ARITH_F16)
    model.set_level(pkg.LEVEL_LOUDNESS, -23.0, -1.0)
    pcm, _, _ = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=60, collect_taps=True)
    levels = model.last_levels()
    for b in range(3):
        y, row = op(pkg, model.tap("waveform", b).ravel(), pkg.LEVEL_LOUDNESS, -23.0, -1.0)
        assert same(pcm[b], y) and same(levels[b], row), b


@pytest.mark.parametrize("rate", (0, 44100))
def test_streamed_chunks_under_a_gain_tile_the_levelled_utterance(pkg, model, ids, rate):
    model.set_level(pkg.LEVEL_GAIN, -4.5)
    model.set_rates(output_rate=rate)
    whole, lengths, frames = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=3)
    levels = model.last_levels()
    assert frames.max() > 40
    chunks = {}
    pcm, l2, _ = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=3, vocoder_chunk_frames=13,
                                     on_chunk=lambda u, off, x: chunks.setdefault(u, []).append((off, x)) and False)
    assert np.array_equal(l2, lengths) and same(model.last_levels(), levels)
    for b in range(3):
        pos = 0
        for off, x in chunks[b]:
            assert off == pos and x.size > 0, (b, off, pos)
            pos += x.size
        assert pos == lengths[b]
        assert same(np.concatenate([x for _, x in chunks[b]]), whole[b]) and same(pcm[b], whole[b]), b
    assert len(chunks[2]) > 1
    if rate == 0:
        model.set_level(pkg.LEVEL_NONE)
        raw, _, _ = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=3)
        g = np.float32(levels[0, 2])
        assert abs(20 * np.log10(float(g)) + 4.5) <= 1e-4 and all(same(whole[b], raw[b] * g) for b in range(3))


@pytest.mark.parametrize("kind", ("LEVEL_MEASURE", "LEVEL_PEAK", "LEVEL_LOUDNESS"))
def test_kinds_that_need_the_whole_utterance_refuse_to_stream(pkg, model, ids, kind):
    model.set_level(getattr(pkg, kind), -20.0, -1.0)
    called = []
    with pytest.raises(pkg.VitsError, match="needs the whole utterance.*only VITS_LEVEL_GAIN streams"):
        model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=3, vocoder_chunk_frames=13, on_chunk=lambda u, off, x: called.append(u) and False)
    assert not called


def test_voice_conversion_delivers_the_operators_levelling(pkg):
    rng = np.random.default_rng(5)
    lens = np.array([16000 // 2, 16000 // 25 + 3], np.int64)
    x = np.full((2, int(lens.max()) + 2), np.nan, np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = 0.3 * rng.standard_normal(n).astype(np.float32)
    with pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_TINY | pkg.SYNTH_POSTERIOR)) as m:
        plain = m.convert_batch(x, lens, noise_seed=3)
        assert m.last_levels() is None
        m.set_level(pkg.LEVEL_LOUDNESS, -30.0, -12.0)
        got = m.convert_batch(x, lens, noise_seed=3, collect_taps=True)
        levels = m.last_levels()
        assert np.array_equal(got[1], plain[1]) and np.array_equal(got[2], plain[2])
        for b in range(2):
            wave = m.tap("waveform", b).ravel()
            assert same(wave, plain[0][b])
            y, row = op(pkg, wave, pkg.LEVEL_LOUDNESS, -30.0, -12.0)
            assert same(got[0][b], y) and same(levels[b], row), b
        print("conversion levels:", levels.tolist())
        assert levels[1, 3] == 0  # (0.04 s: fewer than four segments)


def test_nothing_changes_when_no_level_is_set(pkg, tiny_bytes, ids, plain):
    with pkg.Model(tiny_bytes) as m:
        m.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=60)  # (the first small call makes the latency kernels' weight copy: not the level's doing)
        w0 = m.weight_bytes
        assert m.level == (pkg.LEVEL_NONE, 0.0, 0.0)
        m.set_level(pkg.LEVEL_PEAK, -6.0)
        assert m.weight_bytes == w0  # (nothing is allocated before a call levels)
        m.prof_enable(True)
        m.prof_reset()
        m.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=60)
        report = json.dumps(m.prof_report())
        assert "level_measure" in report and "level_scale" in report
        m.prof_enable(False)
        assert m.last_levels() is not None
        w1 = m.weight_bytes
        assert w1 == w0 + 64 * 4 * 4  # the device row buffer, once
        m.set_level(pkg.LEVEL_NONE)
        m.prof_enable(True)
        m.prof_reset()
        pcm, lengths, _ = m.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=60)
        assert "level_" not in json.dumps(m.prof_report())
        m.prof_enable(False)
        assert m.last_levels() is None
        assert np.array_equal(lengths, plain[60][1]) and all(same(pcm[b], plain[60][0][b]) for b in range(3))
        assert m.weight_bytes == w1
    with pkg.Model(tiny_bytes) as m:  # a handle that never set a level
        m.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=60)
        assert m.weight_bytes == w0


def test_refusals_leave_the_level_as_it_was(pkg, model, ids):
    model.set_level(pkg.LEVEL_PEAK, -2.0)
    for bad in ((9, 0, 0), (-1, 0, 0), (pkg.LEVEL_GAIN, 40.5, 0), (pkg.LEVEL_GAIN, float("nan"), 0), (pkg.LEVEL_PEAK, 1, 0), (pkg.LEVEL_PEAK, -61, 0),
                (pkg.LEVEL_LOUDNESS, -70.5, -1), (pkg.LEVEL_LOUDNESS, -23, 1), (pkg.LEVEL_LOUDNESS, -23, float("-inf"))):
        with pytest.raises(pkg.VitsError, match="vits_model_set_level"):
            model.set_level(*bad)
        assert model.level == (pkg.LEVEL_PEAK, -2.0, 0.0)
    # with a batch in flight
    model.submit_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=3)
    with pytest.raises(pkg.VitsError, match="batches in flight"):
        model.set_level(pkg.LEVEL_GAIN, -3.0)
    model.wait()
    assert model.level == (pkg.LEVEL_PEAK, -2.0, 0.0)
    # from inside on_chunk
    model.set_level(pkg.LEVEL_GAIN, -2.0)
    seen = []

    def sink(u, off, x):
        try:
            model.set_level(pkg.LEVEL_GAIN, -9.0)
        except pkg.VitsError as e:
            seen.append(str(e))
        return False

    model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=3, vocoder_chunk_frames=8, on_chunk=sink)
    assert seen and all("model busy" in s for s in seen)
    assert model.level == (pkg.LEVEL_GAIN, -2.0, 0.0)
