"""A stated pitch at model level (vits_model_set_pitch_ratios, vits_model_set_pitch; include/vits.h "a stated pitch"): the call with a ratio p_b is, bit for bit, the
call with speaking rate r'_b = (float)((double)rate / (double)p_b) followed by the varispeed operator (pkg.pitch) on its waveforms; every entry point
and every way of handing the PCM out gives those bits; the stages behind the vocoder (edges, join, level, limiter, output rate) see the shifted audio;
the report, the taps and the refusals; and with every ratio 1 nothing runs and nothing is allocated.

The tiny model (16 kHz, hop 8), four ragged utterances of at most 24 ids with predicted durations (a pitch refuses fixed_duration), four different ratios,
one of them 1. Every expectation is the operators chained on the waveforms of ONE call without pitch at the rates r'."""
import json

import numpy as np
import pytest

from delivery_helpers import FS, SHAPE, DeviceRows, same
import pitch_ref as PR

pytestmark = pytest.mark.gpu

LENS = np.array([5, 12, 24, 17], np.int32)
RATIOS = np.array([PR.ratio(2), 1.0, PR.ratio(-3), 1.5], np.float32)
RATE = 44100
SENTINEL = 7.25
TRACK = np.array([0, 0, 0, 1], np.int32)
GAPS = np.array([0.0, 12.0, -4.0, 0.0], np.float32)


@pytest.fixture(scope="module")
def ids(pkg):
    return pkg.synth_ids(4, 24)


@pytest.fixture(scope="module")
def tiny(pkg, tiny_bytes):
    with pkg.Model(tiny_bytes) as m:
        assert m.sampling_rate == FS and m.hop == 8 and m.pitch == 1.0
        yield m


def off(m):
    m.set_pitch(1.0)
    m.set_rates(0, 0)
    m.set_level(0)
    m.set_limiter(0)
    m.set_edges(0)


@pytest.fixture()
def model(tiny):
    off(tiny)
    yield tiny
    off(tiny)


def call(m, ids, **kw):
    return m.process_batch(ids, id_lengths=LENS, noise_seed=7, **kw)


def ragged(rows):
    n = np.array([r.size for r in rows], np.int64)
    x = np.zeros((len(rows), int(n.max())), np.float32)
    for b, r in enumerate(rows):
        x[b, :r.size] = r
    return x, n


@pytest.fixture(scope="module")
def refs(pkg, tiny, ids):
    """the chain on the host side of the operators: the call at the rates r' (no pitch), its durations, and the varispeed of its waveforms"""
    off(tiny)
    rate = np.float32(tiny.speaking_rate)
    slow = (np.float64(rate) / RATIOS.astype(np.float64)).astype(np.float32)
    dur = np.zeros((4, 24), np.int32)
    waves, n, frames = call(tiny, ids, speaking_rate=slow, durations_out=dur)
    plain = call(tiny, ids)
    x, lens = ragged(waves)
    y, n_out = pkg.pitch(x, RATIOS, lens)
    rows = [y[b, :n_out[b]].copy() for b in range(4)]
    report = np.array([[pkg.pitch_plan(float(p), int(v))[0], int(v), pkg.pitch_plan(float(p), int(v))[3]] for p, v in zip(RATIOS, n)], np.int64)
    # (spoken slower where p > 1, faster where p < 1)
    assert np.array_equal(report[:, 2], n_out) and frames[0] >= plain[2][0] and frames[3] > plain[2][3] and frames[2] < plain[2][2] and frames[1] == plain[2][1]
    return dict(slow=slow, waves=waves, n=n, frames=frames, dur=dur, plain=plain, rows=rows, n_out=n_out, report=report)


def check(m, result, refs, path, rows=None, n=4):
    pcm, lengths, frames = result
    rows = refs["rows"] if rows is None else rows
    assert np.array_equal(lengths, [r.size for r in rows[:n]]), (path, lengths)
    assert np.array_equal(frames, refs["frames"][:n]), path
    for b in range(n):
        assert same(pcm[b], rows[b]), (path, b)
    assert np.array_equal(m.last_pitch(), refs["report"][:n]), (path, m.last_pitch())


def test_the_call_is_the_slower_call_and_the_operator(pkg, model, ids, refs):
    dur = np.zeros((4, 24), np.int32)
    got = call(model, ids, pitch_ratio=RATIOS, durations_out=dur)
    check(model, got, refs, "pitch_ratios")
    assert np.array_equal(dur, refs["dur"])
    assert np.array_equal(got[1], [PR.plan(float(p), int(v))[4] for p, v in zip(RATIOS, refs["n"])])
    # the row with ratio 1 of the mixed batch is the row of the call without any pitch
    assert same(got[0][1], refs["plain"][0][1]) and got[2][1] == refs["plain"][2][1]
    # frames_only reports the lengths of the full call
    none, lengths, frames = call(model, ids, pitch_ratio=RATIOS, frames_only=True)
    assert none is None and np.array_equal(lengths, got[1]) and np.array_equal(frames, got[2])
    # the taps: "waveform" stays the vocoder's row, "waveform_pitch" is the stage's
    call(model, ids, pitch_ratio=RATIOS, collect_taps=True)
    for b in range(4):
        assert same(model.tap("waveform", b), refs["waves"][b]) and same(model.tap("waveform_pitch", b), refs["rows"][b]), b


def test_every_entry_point_gives_the_same_bits(pkg, model, ids, refs):
    # the model value against the array form (one ratio for the batch)
    p = float(RATIOS[0])
    want = call(model, ids, pitch_ratio=p)
    model.set_pitch(p)
    assert model.pitch == p
    got = call(model, ids)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and all(same(a, b) for a, b in zip(got[0], want[0]))
    one = model.process_ids(ids[0, :LENS[0]])  # (the reference's noise stream: another utterance, but the model value reaches it)
    assert one.size == PR.plan(p, int(model.last_pitch()[0, 1]))[4] and model.last_pitch()[0, 0] == PR.plan(p, 0)[0]
    # an array overrides the model value
    check(model, call(model, ids, pitch_ratio=RATIOS), refs, "array over the model value")
    model.set_pitch(1.0)
    # the pipeline: two batches in flight, each wait reports its own batch
    model.submit_batch(ids, id_lengths=LENS, noise_seed=7, pitch_ratio=RATIOS)
    model.submit_batch(ids[:2], id_lengths=LENS[:2], noise_seed=7, pitch_ratio=RATIOS[:2])
    check(model, model.wait(), refs, "submit / wait")
    check(model, model.wait(), refs, "submit / wait, second batch", n=2)
    # a caller-owned device buffer, no host copy; nothing is written behind a row
    cap = int(refs["n_out"].max()) + 3
    with DeviceRows(4, cap) as dev:
        dev.fill(SENTINEL)
        none, lengths, frames = call(model, ids, pitch_ratio=RATIOS, out_device=dev.ptr, out_device_stride=cap, skip_host_copy=True)
        buf = dev.read()
        assert none is None
        check(model, ([buf[b, :lengths[b]] for b in range(4)], lengths, frames), refs, "out_device")
        for b in range(4):
            assert (buf[b, lengths[b]:] == SENTINEL).all(), ("written past the row", b)
    # vocoder windows without a sink: the stage runs behind the last window
    assert refs["frames"].max() > 3 * 7
    check(model, call(model, ids, pitch_ratio=RATIOS, vocoder_chunk_frames=7), refs, "windows")


@pytest.mark.parametrize("lv", ("loudness+limiter", "gain+limiter"))
def test_the_stages_behind_see_the_shifted_audio(pkg, model, ids, refs, lv):
    """edges, a level under the limiter and an output rate behind the pitch stage: the delivery is the operators chained on the shifted rows"""
    desc = dict(SHAPE, mode=pkg.EDGES_TRIM_RELATIVE, threshold_db=-1.0)
    x, n = ragged(refs["rows"])
    y, n1, ed_rows = pkg.edges(x, FS, lens=n, **desc)
    trimmed = [y[b, :n1[b]].copy() for b in range(4)]
    ceiling = float(np.float32(20.0 * np.log10(float(np.abs(trimmed[2]).max())) - 6.0))
    kind, value = (pkg.LEVEL_LOUDNESS, -20.0) if lv.startswith("loudness") else (pkg.LEVEL_GAIN, 3.0)
    x, n = ragged(trimmed)
    y, levels, limits = pkg.limit(x, FS, kind, value, ceiling, lens=n)
    x, n = ragged([y[b, :n[b]] for b in range(4)])
    y, n_out = pkg.resample(x, FS, RATE, lens=n)
    want = [y[b, :n_out[b]].copy() for b in range(4)]
    model.set_limiter(pkg.LIMIT_TRUE_PEAK)
    model.set_level(kind, value, ceiling)
    model.set_edges(**desc)
    model.set_rates(0, RATE)
    for path, kw in (("sync", {}), ("windows", dict(vocoder_chunk_frames=7))):
        check(model, call(model, ids, pitch_ratio=RATIOS, **kw), refs, path, rows=want)
        assert np.array_equal(model.last_edges(), ed_rows) and same(model.last_levels(), levels) and same(model.last_limits(), limits), path
    model.submit_batch(ids, id_lengths=LENS, noise_seed=7, pitch_ratio=RATIOS)
    check(model, model.wait(), refs, "submit / wait", rows=want)
    assert np.array_equal(model.last_edges(), ed_rows) and same(model.last_levels(), levels)
    # frames_only: the bounds of the full call at the output rate
    none, lengths, _ = call(model, ids, pitch_ratio=RATIOS, frames_only=True)
    pads = int(n1[0] - ed_rows[0, 1] + ed_rows[0, 0])  # (Pl + Pt)
    assert np.array_equal(lengths, [pkg.resample_length(FS, RATE, int(v) + pads) for v in refs["n_out"]])


def test_a_joined_call_mixes_pitches_on_one_track(pkg, model, ids, refs):
    x, n = ragged(refs["rows"])
    y, tl, on = pkg.join(x, FS, lens=n, track=TRACK, gap_ms=GAPS)
    tracks = [y[g, :tl[g]].copy() for g in range(2)]
    x, n = ragged(tracks)
    y, levels = pkg.level(x, FS, pkg.LEVEL_GAIN, -3.0, lens=n)
    x, n = ragged([y[g, :n[g]] for g in range(2)])
    y, n_out = pkg.resample(x, FS, RATE, lens=n)
    model.set_level(pkg.LEVEL_GAIN, -3.0)
    model.set_rates(0, RATE)
    kw = dict(id_lengths=LENS, track=TRACK, gap_ms=GAPS, noise_seed=7, pitch_ratio=RATIOS)
    pcm, lengths, frames = model.process_joined(ids, **kw)
    assert np.array_equal(lengths, n_out) and frames.tolist() == [int(refs["frames"][:3].sum()), int(refs["frames"][3])]
    for g in range(2):
        assert same(pcm[g], y[g, :n_out[g]]), g
    assert np.array_equal(model.last_joins()[:, 2:], on) and np.array_equal(model.last_pitch(), refs["report"])
    # frames_only: the tracks' bounds, from N'
    _, bounds, _ = model.process_joined(ids, frames_only=True, **kw)
    G, jb, _ = pkg.join_plan(FS, refs["n_out"], TRACK, GAPS)
    assert np.array_equal(bounds, [pkg.resample_length(FS, RATE, int(v)) for v in jb])


def test_refusals(pkg, model, ids, refs):
    called = []
    sink = dict(vocoder_chunk_frames=7, on_chunk=lambda u, o, x: called.append(u) and False)
    with pytest.raises(pkg.VitsError, match="on_chunk.*pitch ratio other than 1.*streaming pitch is not built"):
        call(model, ids, pitch_ratio=RATIOS, **sink)
    with pytest.raises(pkg.VitsError, match="async.*pitch ratio other than 1.*streaming pitch is not built"):
        call(model, ids, pitch_ratio=RATIOS, skip_host_copy=True, async_=True)
    model.set_pitch(float(RATIOS[0]))
    with pytest.raises(pkg.VitsError, match="on_chunk.*streaming pitch is not built"):
        call(model, ids, **sink)
    with pytest.raises(pkg.VitsError, match="vits_model_process_joined: on_chunk"):
        model.process_joined(ids, id_lengths=LENS, **sink)
    model.set_pitch(1.0)
    assert not called
    with pytest.raises(pkg.VitsError, match=r"utterance 0 has the pitch ratio .*fixed_duration > 0"):
        call(model, ids, pitch_ratio=RATIOS, fixed_duration=3)
    ovr = np.full((4, 24), -1, np.int32)
    call(model, ids, pitch_ratio=RATIOS, duration_override=ovr)  # (nothing stated: taken)
    ovr[1, 3] = 2
    call(model, ids, pitch_ratio=RATIOS, duration_override=ovr)  # (stated on the utterance with ratio 1: taken)
    ovr[2, 4] = 2
    with pytest.raises(pkg.VitsError, match=r"utterance 2 has the pitch ratio .*duration_override states token 4"):
        call(model, ids, pitch_ratio=RATIOS, duration_override=ovr)
    for bad in (np.nan, 0.49, 2.01):
        r = RATIOS.copy()
        r[3] = bad
        with pytest.raises(pkg.VitsError, match=r"pitch_ratios\[3\] = .*must be finite and in \[0.5, 2\]"):
            call(model, ids, pitch_ratio=r)
        with pytest.raises(pkg.VitsError, match=r"vits_model_set_pitch: .*outside \[0.5, 2\]"):
            model.set_pitch(bad)
    assert model.pitch == 1.0
    # r' = rate / p must stay a speaking rate
    with pytest.raises(pkg.VitsError, match=r"utterance 2 has the pitch ratio 0.5.*becomes 12, outside \[0.1, 10\]"):
        call(model, ids, pitch_ratio=[1.0, 1.0, 0.5, 1.0], speaking_rate=6.0)
    with pytest.raises(pkg.VitsError, match=r"utterance 0 has the pitch ratio 2.*outside \[0.1, 10\]"):
        call(model, ids, pitch_ratio=2.0, speaking_rate=0.15)
    # the text entry point takes the model value only
    with pytest.raises(pkg.VitsError, match="vits_model_speak: the ratios of vits_model_set_pitch_ratios are one per utterance"):
        model.speak("a b. c d.", pitch_ratio=RATIOS[:1])
    # conversion and alignment have no durations to stretch
    pcm = refs["plain"][0][2]
    with pytest.raises(pkg.VitsError, match="voice conversion does not take the ratios of vits_model_set_pitch_ratios"):
        model.convert_batch(pcm, pitch_ratio=1.5)
    with pytest.raises(pkg.VitsError, match="alignment does not take the ratios of vits_model_set_pitch_ratios"):
        model.align_batch(pcm, ids[2], pitch_ratio=1.5)
    # a call that fails in the wrapper, before the library is reached, leaves no ratios behind for a later call
    with pytest.raises(TypeError, match="unknown arguments"):
        model.convert_batch(pcm, pitch_ratio=1.5, no_such_argument=1)
    with pytest.raises(ValueError, match="pitch_ratio needs a scalar or one value per utterance"):
        call(model, ids, pitch_ratio=RATIOS[:3])
    assert call(model, ids)[1].tolist() == refs["plain"][1].tolist() and model.last_pitch() is None
    # ratios are taken by the next call alone, and their count is the call's batch
    model.set_pitch_ratios(RATIOS[:3])
    with pytest.raises(pkg.VitsError, match="vits_model_set_pitch_ratios gave 3 ratios, and this call has 4 utterances"):
        call(model, ids)
    got = call(model, ids)  # (gone with the refused call: the plain call)
    assert model.last_pitch() is None and all(same(a, b) for a, b in zip(got[0], refs["plain"][0]))
    model.set_pitch_ratios(RATIOS)
    model.set_pitch_ratios(None)
    assert call(model, ids)[1].tolist() == refs["plain"][1].tolist() and model.last_pitch() is None
    # the handle still delivers
    check(model, call(model, ids, pitch_ratio=RATIOS), refs, "after the refusals")
    assert call(model, ids)[1].tolist() == refs["plain"][1].tolist() and model.last_pitch() is None  # (and the call after it is plain again)


def test_with_every_ratio_one_nothing_runs(pkg, tiny_bytes, ids, refs):
    """a fresh handle: the call without pitch, then the call with ratios of 1 (array and model value): the same bits, no pitch launch in the profiler's
    report, no report rows, and vits_model_weight_bytes as after the plain call; the first call that shifts then uploads the table (64 KiB + 16 bytes)"""
    with pkg.Model(tiny_bytes) as m:
        plain = call(m, ids)
        weight = m.weight_bytes
        for b in range(4):
            assert same(plain[0][b], refs["plain"][0][b])
        m.set_pitch(1.0)
        m.prof_enable()
        m.prof_reset()
        got = call(m, ids, pitch_ratio=np.ones(4, np.float32))
        assert '"pitch"' not in json.dumps(m.prof_report())
        m.prof_enable(False)
        assert np.array_equal(got[1], plain[1]) and all(same(a, b) for a, b in zip(got[0], plain[0]))
        assert m.last_pitch() is None and m.weight_bytes == weight
        m.prof_enable()
        m.prof_reset()
        call(m, ids, pitch_ratio=RATIOS)
        assert '"pitch"' in json.dumps(m.prof_report())
        m.prof_enable(False)
        assert m.weight_bytes == weight + 8 * (PR.ZQ + 2)
        call(m, ids, pitch_ratio=RATIOS)
        assert m.weight_bytes == weight + 8 * (PR.ZQ + 2)
