"""A conversion's rate and pitch at model level (vits_model_set_conversion_ratios, vits_model_set_conversion_prosody; include/vits.h "a stated tempo"): the
conversion with rate r_b and pitch p_b is, bit for bit, the plain conversion followed by the time-stretch operator (pkg.tempo) at q_b = (float)((double)r_b /
(double)p_b) and then the varispeed operator (pkg.pitch) at p_b; every way of handing the PCM out gives those bits; the stages behind (edges, level, limiter,
output rate) see the final audio; the report, the taps and the refusals; and with every value 1 nothing runs and nothing is allocated.

The tiny multi-speaker model with a posterior encoder (16 kHz, hop 8), four recordings of 200 to 400 frames. Every expectation is the operators chained on the
waveforms of ONE plain conversion of the session."""
import json

import numpy as np
import pytest

from delivery_helpers import FS, SHAPE, DeviceRows, same

pytestmark = pytest.mark.gpu

N = np.array([2400, 1603, 3201, 2000], np.int64)
SRC, TGT = [0, 1, 0, 1], [1, 0, 1, 0]
P2, PM3 = float(np.float32(2.0 ** (2 / 12))), float(np.float32(2.0 ** (-3 / 12)))
CASES = {
    "rate 0.8": ([0.8] * 4, [1.0] * 4),
    "pitch +2": ([1.0] * 4, [P2] * 4),
    "rate 1.25, pitch -3": ([1.25] * 4, [PM3] * 4),
    "rate 1.5, pitch 1.5": ([1.5] * 4, [1.5] * 4),
    "mix": ([0.8, 1.0, 1.25, 1.0], [1.0, P2, PM3, 1.0]),
}
RATE = 44100
SENTINEL = 7.25


def recordings():
    rng = np.random.default_rng(5)
    out = np.zeros((N.size, int(N.max())), np.float32)
    for b, n in enumerate(N):
        t = np.arange(n) / FS
        y = np.sin(2 * np.pi * rng.uniform(100, 250) * t) + 0.3 * np.sin(2 * np.pi * rng.uniform(400, 900) * t) + 0.05 * rng.standard_normal(n)
        out[b, :n] = 0.8 * y / np.abs(y).max()
    return out


@pytest.fixture(scope="module")
def tiny(pkg):
    with pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_TINY | pkg.SYNTH_SPEAKERS | pkg.SYNTH_POSTERIOR)) as m:
        assert m.sampling_rate == FS and m.hop == 8 and m.conversion_prosody == (1.0, 1.0)
        yield m


def off(m):
    m.set_conversion_prosody(1.0, 1.0)
    m.set_rates(0, 0)
    m.set_level(0)
    m.set_limiter(0)
    m.set_edges(0)


@pytest.fixture()
def model(tiny):
    off(tiny)
    yield tiny
    off(tiny)


def call(m, pcm, **kw):
    return m.convert_batch(pcm, N, src=SRC, tgt=TGT, noise_seed=7, **kw)


def ragged(rows):
    n = np.array([r.size for r in rows], np.int64)
    x = np.zeros((len(rows), int(n.max())), np.float32)
    for b, r in enumerate(rows):
        x[b, :r.size] = r
    return x, n


def chain(pkg, waves, rates, pitches):
    """the operators on the plain conversion's waveforms: (final rows, the stretched rows, last_tempo's rows or None, last_pitch's rows or None)"""
    r, p = np.asarray(rates, np.float32), np.asarray(pitches, np.float32)
    q = (r.astype(np.float64) / p.astype(np.float64)).astype(np.float32)
    x, n = ragged(waves)
    y, n1, _ = pkg.tempo(x, FS, q, n)
    stretched = [y[b, :n1[b]].copy() for b in range(len(waves))]
    tempo_rows = None
    if (q != 1).any():
        tempo_rows = np.array([[pkg.tempo_plan(FS, float(qb), int(v))[2], int(v), int(v1), pkg.tempo_plan(FS, float(qb), int(v))[3]] for qb, v, v1 in zip(q, n, n1)], np.int64)
    rows, pitch_rows = stretched, None
    if (p != 1).any():
        x, n = ragged(stretched)
        y, n2 = pkg.pitch(x, p, n)
        rows = [y[b, :n2[b]].copy() for b in range(len(waves))]
        pitch_rows = np.array([[pkg.pitch_plan(float(pb), int(v))[0], int(v), int(v2)] for pb, v, v2 in zip(p, n, n2)], np.int64)
    return rows, stretched, tempo_rows, pitch_rows


@pytest.fixture(scope="module")
def refs(pkg, tiny):
    """ONE plain conversion of the session, and the chained operators of every case on its waveforms"""
    off(tiny)
    pcm = recordings()
    waves, n, frames = call(tiny, pcm)
    assert tiny.last_tempo() is None and tiny.last_pitch() is None
    assert np.array_equal(frames, N // 8) and frames.min() >= 200
    for w in waves:
        w.setflags(write=False)
    return dict(pcm=pcm, waves=waves, n=n, frames=frames, cases={k: chain(pkg, waves, r, p) for k, (r, p) in CASES.items()})


def reports_equal(m, tempo_rows, pitch_rows):
    a, b = m.last_tempo(), m.last_pitch()
    return ((a is None) if tempo_rows is None else np.array_equal(a, tempo_rows)) and ((b is None) if pitch_rows is None else np.array_equal(b, pitch_rows))


def check(m, result, refs, case, path, rows=None):
    pcm, lengths, frames = result
    final, _, tempo_rows, pitch_rows = refs["cases"][case]
    rows = final if rows is None else rows
    assert np.array_equal(lengths, [r.size for r in rows]), (case, path, lengths)
    assert np.array_equal(frames, refs["frames"]), (case, path)
    for b in range(4):
        assert same(pcm[b], rows[b]), (case, path, b)
    assert reports_equal(m, tempo_rows, pitch_rows), (case, path, m.last_tempo(), m.last_pitch())


@pytest.mark.parametrize("case", CASES)
def test_the_conversion_is_the_plain_one_and_the_operators(pkg, model, refs, case):
    rates, pitches = CASES[case]
    final, stretched, tempo_rows, pitch_rows = refs["cases"][case]
    kw = dict(vc_rate=rates, vc_pitch=pitches)
    got = call(model, refs["pcm"], **kw)
    check(model, got, refs, case, "host")
    # N' of the two plans, chained
    for b in range(4):
        q = float(np.float32(np.float64(np.float32(rates[b])) / np.float64(np.float32(pitches[b]))))
        n1 = pkg.tempo_plan(FS, q, int(refs["n"][b]))[4]
        assert got[1][b] == pkg.pitch_plan(pitches[b], n1)[3]
    # a row with rate and pitch 1 of the mixed batch is the plain conversion's row
    for b in range(4):
        if rates[b] == 1.0 and pitches[b] == 1.0:
            assert same(got[0][b], refs["waves"][b])
    # vocoder windows without a sink: the stages run behind the last window
    check(model, call(model, refs["pcm"], vocoder_chunk_frames=7, **kw), refs, case, "windows")
    # a caller-owned device buffer, no host copy; nothing is written behind a row; and the device's PCM16 of it
    cap = max(r.size for r in final) + 3
    with DeviceRows(4, cap) as dev, DeviceRows(4, cap) as dev16:
        dev.fill(SENTINEL)
        none, lengths, frames = call(model, refs["pcm"], out_device=dev.ptr, out_device_stride=cap, skip_host_copy=True, **kw)
        buf = dev.read()
        assert none is None
        check(model, ([buf[b, :lengths[b]] for b in range(4)], lengths, frames), refs, case, "out_device")
        for b in range(4):
            assert (buf[b, lengths[b]:] == SENTINEL).all(), ("written past the row", b)
        pkg.pcm16_device(dev.ptr, cap, dev16.ptr, 2 * cap, 4, cap)
        shorts = dev16.read().view(np.int16)
        for b in range(4):
            assert np.array_equal(shorts[b, :lengths[b]], pkg.pcm16(final[b])), (case, "PCM16", b)
            assert np.array_equal(pkg.pcm16(got[0][b]), pkg.pcm16(final[b]))
    if case == "mix":
        # the taps: "waveform" stays the vocoder's row, "waveform_tempo" is the stretch's, "waveform_pitch" the varispeed's behind it
        call(model, refs["pcm"], collect_taps=True, **kw)
        for b in range(4):
            assert same(model.tap("waveform", b), refs["waves"][b]) and same(model.tap("waveform_tempo", b), stretched[b]), b
            assert same(model.tap("waveform_pitch", b), final[b]), b
        # the model value against the array form, and the one-utterance entry point
        model.set_conversion_prosody(0.8, P2)
        assert model.conversion_prosody == (float(np.float32(0.8)), P2)
        a = call(model, refs["pcm"])
        w = call(model, refs["pcm"], vc_rate=0.8, vc_pitch=P2)
        assert np.array_equal(a[1], w[1]) and all(same(x, y) for x, y in zip(a[0], w[0])) and a[1][0] != refs["n"][0]
        # an array overrides the model value
        check(model, call(model, refs["pcm"], **kw), refs, case, "arrays over the model value")
        model.set_conversion_prosody(1.0, 1.0)
        one = model.convert(refs["pcm"][0, :N[0]], SRC[0], TGT[0], vc_rate=0.8)
        assert one.size == pkg.tempo_plan(FS, 0.8, int(model.last_tempo()[0, 1]))[4] and model.last_tempo()[0, 0] == pkg.tempo_plan(FS, 0.8, 0)[2]


@pytest.mark.parametrize("case", CASES)
def test_the_stages_behind_see_the_final_audio(pkg, model, refs, case):
    """edges, a loudness level under the limiter and an output rate behind the two stages: the delivery is the operators chained on the final rows"""
    rates, pitches = CASES[case]
    final = refs["cases"][case][0]
    desc = dict(SHAPE, mode=pkg.EDGES_TRIM_RELATIVE, threshold_db=-1.0)
    x, n = ragged(final)
    y, n1, ed_rows = pkg.edges(x, FS, lens=n, **desc)
    trimmed = [y[b, :n1[b]].copy() for b in range(4)]
    ceiling = float(np.float32(20.0 * np.log10(float(np.abs(trimmed[2]).max())) - 6.0))
    x, n = ragged(trimmed)
    y, levels, limits = pkg.limit(x, FS, pkg.LEVEL_LOUDNESS, -20.0, ceiling, lens=n)
    x, n = ragged([y[b, :n[b]] for b in range(4)])
    y, n_out = pkg.resample(x, FS, RATE, lens=n)
    want = [y[b, :n_out[b]].copy() for b in range(4)]
    model.set_limiter(pkg.LIMIT_TRUE_PEAK)
    model.set_level(pkg.LEVEL_LOUDNESS, -20.0, ceiling)
    model.set_edges(**desc)
    model.set_rates(0, RATE)
    for path, kw in (("sync", {}), ("windows", dict(vocoder_chunk_frames=7))):
        check(model, call(model, refs["pcm"], vc_rate=rates, vc_pitch=pitches, **kw), refs, case, path, rows=want)
        assert np.array_equal(model.last_edges(), ed_rows) and same(model.last_levels(), levels) and same(model.last_limits(), limits), path


def test_refusals(pkg, model, refs):
    pcm = refs["pcm"]
    called = []
    sink = dict(vocoder_chunk_frames=7, on_chunk=lambda u, o, x: called.append(u) and False)
    with pytest.raises(pkg.VitsError, match=r"utterance 2: on_chunk.*conversion rate 1\.25"):
        call(model, pcm, vc_rate=[1.0, 1.0, 1.25, 1.0], **sink)
    with pytest.raises(pkg.VitsError, match=r"utterance 0: on_chunk.*pitch 1\.5"):
        call(model, pcm, vc_rate=1.5, vc_pitch=1.5, **sink)
    model.set_conversion_prosody(0.8, 1.0)
    with pytest.raises(pkg.VitsError, match="utterance 0: on_chunk"):
        call(model, pcm, **sink)
    model.set_conversion_prosody(1.0, 1.0)
    assert not called
    call(model, pcm, vc_rate=1.0, vc_pitch=1.0, **sink)  # (every value 1: streams as ever)
    assert called
    for bad in (np.nan, np.inf, 0.49, 2.01):
        r = np.ones(4, np.float32)
        r[3] = bad
        with pytest.raises(pkg.VitsError, match=r"utterance 3: conversion rate .* is not finite or outside \[0.5, 2\]"):
            call(model, pcm, vc_rate=r)
        with pytest.raises(pkg.VitsError, match=r"utterance 3: conversion pitch .* is not finite or outside \[0.5, 2\]"):
            call(model, pcm, vc_pitch=r)
        with pytest.raises(pkg.VitsError, match=r"vits_model_set_conversion_prosody: rate .*outside \[0.5, 2\]"):
            model.set_conversion_prosody(bad, 1.0)
        with pytest.raises(pkg.VitsError, match=r"vits_model_set_conversion_prosody: pitch .*outside \[0.5, 2\]"):
            model.set_conversion_prosody(1.0, bad)
    assert model.conversion_prosody == (1.0, 1.0)
    # r and p in range, q = r / p not
    with pytest.raises(pkg.VitsError, match=r"utterance 1: conversion rate 2 over pitch 0\.75 is the tempo .*outside \[0.5, 2\]"):
        call(model, pcm, vc_rate=[1.0, 2.0, 1.0, 1.0], vc_pitch=[1.0, 0.75, 1.0, 1.0])
    with pytest.raises(pkg.VitsError, match=r"utterance 0: conversion rate 0\.5 over pitch 1\.5"):
        call(model, pcm, vc_rate=0.5, vc_pitch=1.5)
    # another count of pairs than utterances
    model.set_conversion_ratios([0.8, 0.8, 0.8], None)
    with pytest.raises(pkg.VitsError, match="vits_model_set_conversion_ratios gave 3 pairs, and this call has 4 utterances"):
        call(model, pcm)
    got = call(model, pcm)  # (gone with the refused call: the plain conversion)
    assert model.last_tempo() is None and all(same(a, b) for a, b in zip(got[0], refs["waves"]))
    with pytest.raises(ValueError, match="vc_rate and vc_pitch need a scalar or one value per utterance"):
        call(model, pcm, vc_rate=[0.8, 0.8, 0.8])
    # a call that fails in the wrapper, before the library is reached, leaves no pairs behind for a later call
    with pytest.raises(TypeError, match="unknown arguments"):
        call(model, pcm, vc_rate=0.8, no_such_argument=1)
    assert all(same(a, b) for a, b in zip(call(model, pcm)[0], refs["waves"])) and model.last_tempo() is None
    # what a conversion refused before, it refuses now, in the same words
    with pytest.raises(pkg.VitsError, match="voice conversion does not take the ratios of vits_model_set_pitch_ratios"):
        call(model, pcm, pitch_ratio=1.5)
    with pytest.raises(pkg.VitsError, match=r"voice conversion does not take opts\.speaking_rates"):
        call(model, pcm, speaking_rate=1.5)
    with pytest.raises(pkg.VitsError, match="voice conversion does not take async"):
        call(model, pcm, vc_rate=0.8, skip_host_copy=True, async_=True)
    # ... and the model's TTS pitch has no effect on a conversion
    model.set_pitch(1.5)
    got = call(model, pcm)
    model.set_pitch(1.0)
    assert model.last_pitch() is None and all(same(a, b) for a, b in zip(got[0], refs["waves"]))
    # the handle still delivers
    check(model, call(model, pcm, vc_rate=CASES["mix"][0], vc_pitch=CASES["mix"][1]), refs, "mix", "after the refusals")
    assert all(same(a, b) for a, b in zip(call(model, pcm)[0], refs["waves"])) and model.last_tempo() is None  # (and the call after it is plain again)


def test_pairs_are_taken_by_the_next_conversion_alone(pkg, model, refs):
    pcm = refs["pcm"]
    rates, pitches = CASES["mix"]
    model.set_conversion_ratios(rates, pitches)
    # a text-to-speech call in between leaves them where they are (and stretches nothing)
    ids = pkg.synth_ids(1, 12)
    tts = model.process_batch(ids, noise_seed=7)
    assert model.last_tempo() is None and model.last_pitch() is None
    again = model.process_batch(ids, noise_seed=7)
    assert same(tts[0][0], again[0][0])
    dur = model.align_batch(pcm[0, :N[0]], ids[0], speakers=SRC[0])  # (nor does an alignment take them)
    assert dur[1][0] == N[0] // 8
    check(model, call(model, pcm), refs, "mix", "the pairs given before the TTS call")
    got = call(model, pcm)  # (taken by that conversion: this one is plain)
    assert model.last_tempo() is None and model.last_pitch() is None and all(same(a, b) for a, b in zip(got[0], refs["waves"]))
    # rates alone, pitches alone: the other side is the model value
    model.set_conversion_ratios(CASES["rate 0.8"][0], None)
    check(model, call(model, pcm), refs, "rate 0.8", "rates alone")
    model.set_conversion_ratios(None, CASES["pitch +2"][1])
    check(model, call(model, pcm), refs, "pitch +2", "pitches alone")
    # given and dropped
    model.set_conversion_ratios(rates, pitches)
    model.set_conversion_ratios(None, None)
    assert all(same(a, b) for a, b in zip(call(model, pcm)[0], refs["waves"])) and model.last_tempo() is None


def test_with_every_value_one_nothing_runs(pkg, refs):
    """a fresh handle: the plain conversion (the recorded call's bits), then the conversion with rates and pitches of 1 (arrays and model values): the same bits,
    no tempo or pitch launch in the profiler's report and the launches of the plain call, no report rows, and vits_model_weight_bytes as after the plain call; a
    conversion that stretches then lists the two launches and still owns nothing more (the stage keeps no table on the device)"""
    pcm = refs["pcm"]
    with pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_TINY | pkg.SYNTH_SPEAKERS | pkg.SYNTH_POSTERIOR)) as m:
        m.prof_enable()
        m.prof_reset()
        plain = call(m, pcm)
        plain_report = m.prof_report()
        m.prof_enable(False)
        weight = m.weight_bytes
        for b in range(4):
            assert same(plain[0][b], refs["waves"][b])
        m.set_conversion_prosody(1.0, 1.0)
        m.prof_enable()
        m.prof_reset()
        got = call(m, pcm, vc_rate=np.ones(4, np.float32), vc_pitch=np.ones(4, np.float32))
        report = m.prof_report()
        m.prof_enable(False)
        names = lambda rep: sorted(set(__import__("re").findall(r'"name": "([^"]+)"', json.dumps(rep))))
        assert '"tempo_' not in json.dumps(report) and '"pitch"' not in json.dumps(report)
        assert names(report) == names(plain_report)
        assert np.array_equal(got[1], plain[1]) and all(same(a, b) for a, b in zip(got[0], plain[0]))
        assert m.last_tempo() is None and m.last_pitch() is None and m.weight_bytes == weight
        m.prof_enable()
        m.prof_reset()
        call(m, pcm, vc_rate=0.8)
        text = json.dumps(m.prof_report())
        m.prof_enable(False)
        assert '"tempo_search"' in text and '"tempo_ola"' in text and '"pitch"' not in text
        assert m.weight_bytes == weight and m.last_tempo().shape == (4, 4)
