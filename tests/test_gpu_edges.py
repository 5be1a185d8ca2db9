"""Stated edges through the engine (vits_model_set_edges, edges.hip): what a call delivers and reports is the operator (vits_op_edges) applied to the
model-rate waveform, bit for bit, through every way a call can deliver it (batch rows, the pipeline, a split batch, vocoder windows, a device buffer,
16-bit arithmetic, voice conversion); the stage comes before levelling, the limiter and the resampler; nothing changes with it off; the refusals.

The threshold. The synthetic models make stationary noise with no silence in it: the 10 ms windows of an utterance lie within a few dB of its loudest.
The tests therefore trim with TRIM_RELATIVE and a small drop: from the plain waveforms, the first threshold_db of (-0.5, -1, -1.5, -2, -3) for which the
restatement (tests/edges_ref.py) moves a or b on at least two of the three utterances with margin >= 1e-6 on all of them; one must exist."""
import ctypes as C
import json

import numpy as np
import pytest

import edges_ref as ER
from delivery_helpers import FS, LENS, MARGIN, PADS, SHAPE, choose, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ids(pkg):
    return pkg.synth_ids(3, 31)


@pytest.fixture(scope="module")
def tiny(pkg, tiny_bytes):
    with pkg.Model(tiny_bytes) as m:
        assert m.sampling_rate == FS and m.hop == 8
        yield m


@pytest.fixture(scope="module")
def plain(pkg, tiny, ids):
    """the calls with the stage off, at fixed_duration 60 and 200: (pcm, lengths, frames, durations)"""
    tiny.set_edges(pkg.EDGES_OFF)
    out = {}
    for fd in (60, 200):
        d = np.zeros(ids.shape, np.int32)
        pcm, lengths, frames = tiny.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=fd, durations_out=d)
        assert tiny.last_edges() is None
        out[fd] = (pcm, lengths, frames, d)
    return out


@pytest.fixture(scope="module")
def desc(pkg, plain):
    """fd -> the desc the tests of that duration use"""
    out = {}
    for fd in (60, 200):
        th = choose(plain[fd][0])
        assert th is not None, fd
        out[fd] = dict(SHAPE, mode=pkg.EDGES_TRIM_RELATIVE, threshold_db=th)
    return out


@pytest.fixture(scope="module")
def trimmed(pkg, plain, desc):
    """the anchor of the tests below: the operator on the plain waveforms, computed once: fd -> [(y [N'], row [4])]"""
    out = {}
    for fd in (60, 200):
        out[fd] = []
        for w in plain[fd][0]:
            assert ER.margin(w, FS, ER.TRIM_RELATIVE, desc[fd]["threshold_db"], **SHAPE) >= MARGIN
            y, n1, rows = pkg.edges(w, FS, **desc[fd])
            want_y, want_row = ER.edges(w, FS, ER.TRIM_RELATIVE, desc[fd]["threshold_db"], **SHAPE)
            assert np.array_equal(rows[0], want_row) and n1[0] == want_row[2] and same(y[0, :n1[0]], want_y)
            out[fd].append((y[0, :n1[0]].copy(), rows[0].copy()))
    return out


@pytest.fixture()
def model(pkg, tiny):
    """the shared handle; stage off, no level, no limiter, at the model's rate and fp32 afterwards"""
    yield tiny
    tiny.set_arith(pkg.ARITH_F32)
    tiny.set_rates(0, 0)
    tiny.set_level(pkg.LEVEL_NONE)
    tiny.set_limiter(pkg.LIMIT_OFF)
    tiny.set_edges(pkg.EDGES_OFF)


@pytest.mark.parametrize("fd", (60, 200))
def test_a_call_delivers_and_reports_the_operators_edges(pkg, model, ids, plain, desc, trimmed, fd):
    model.set_edges(**desc[fd])
    got = model.edges
    assert got["mode"] == pkg.EDGES_TRIM_RELATIVE and got["threshold_db"] == np.float32(desc[fd]["threshold_db"]) and got["tail_ms"] == 30.0
    d = np.zeros(ids.shape, np.int32)
    pcm, lengths, frames = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=fd, durations_out=d, collect_taps=True)
    rows = model.last_edges()
    p = plain[fd]
    assert rows.shape == (3, 4) and rows.dtype == np.int64
    assert np.array_equal(frames, p[2]) and np.array_equal(d, p[3])  # frames[] and durations_out are unchanged
    for b in range(3):
        wave = model.tap("waveform", b).ravel()
        assert same(wave, p[0][b])  # (the model-rate waveform is what it was)
        y, row = trimmed[fd][b]
        assert np.array_equal(rows[b], row) and lengths[b] == row[2] == y.size, (b, rows[b], row)
        assert same(pcm[b], y), b
        assert same(model.tap("waveform_edges", b).ravel(), y), b
        assert row[2] == PADS + row[1] - row[0] and not pcm[b][:320].any() and not pcm[b][-480:].any()
    assert sum(int(r[0] > 0 or r[1] < w.size) for (_, r), w in zip(trimmed[fd], p[0])) >= 2  # the stage does trim here
    print("rows:", rows.tolist())
    # frames_only: lengths[] for the bound N + Pl + Pt, the size to allocate
    _, bound, f0 = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=fd, frames_only=True)
    assert np.array_equal(bound, p[1] + PADS) and np.array_equal(f0, p[2]) and (lengths <= bound).all()
    # PAD: exact
    model.set_edges(pkg.EDGES_PAD, **SHAPE)
    pcm, lengths, _ = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=fd)
    assert np.array_equal(lengths, bound) and model.last_edges()[:, :2].tolist() == [[0, int(n)] for n in p[1]] and not model.last_edges()[:, 3].any()
    for b in range(3):
        assert same(pcm[b], ER.edges(p[0][b], FS, ER.PAD, **SHAPE)[0]), b


def test_the_stage_comes_before_levelling_the_limiter_and_the_resampler(pkg, model, ids, plain, desc, trimmed):
    fd = 200
    model.set_edges(**desc[fd])
    model.set_limiter(pkg.LIMIT_TRUE_PEAK)
    # (in range for a tanh output: the loudness of the trimmed utterance 2, 3 s long, under a ceiling 6 dB below its peak, so that the limiter works in earnest)
    y0 = trimmed[fd][2][0]
    value = float(np.float32(pkg.loudness_host(y0, FS)[0]))
    ceiling = float(np.float32(20.0 * np.log10(float(np.abs(y0).max())) - 6.0))
    assert -70 <= value <= 0 and -60 <= ceiling <= 0
    model.set_level(pkg.LEVEL_LOUDNESS, value, ceiling)
    model.set_rates(output_rate=44100)
    pcm, lengths, _ = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=fd, collect_taps=True)
    for b in range(3):
        y, row = trimmed[fd][b]
        assert same(model.tap("waveform_edges", b).ravel(), y) and np.array_equal(model.last_edges()[b], row)
        yl, levels, limits = pkg.limit(y, FS, pkg.LEVEL_LOUDNESS, value, ceiling)
        assert same(model.last_levels()[b], levels[0]) and same(model.last_limits()[b], limits[0]), b  # they describe the trimmed row
        assert same(model.tap("waveform_level", b).ravel(), yl[0, :y.size]), b
        out, n = pkg.resample(yl[0, :y.size], FS, 44100)
        assert lengths[b] == n[0] == pkg.resample_length(FS, 44100, int(row[2])) and same(pcm[b], out[0, :n[0]]), b
        assert same(model.tap("waveform_out", b).ravel(), out[0, :n[0]]), b
    assert model.last_limits()[2, 2] < 0.75
    # frames_only at the output rate: the bound, resampled
    _, bound, _ = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=fd, frames_only=True)
    assert [int(v) for v in bound] == [pkg.resample_length(FS, 44100, int(n) + PADS) for n in plain[fd][1]]
    # the level alone (no limiter), measured only, at the model's rate
    model.set_rates(0, 0)
    model.set_limiter(pkg.LIMIT_OFF)
    model.set_level(pkg.LEVEL_MEASURE)
    pcm, lengths, _ = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=fd)
    for b in range(3):
        y, row = trimmed[fd][b]
        assert same(pcm[b], y) and same(model.last_levels()[b], pkg.level(y, FS, pkg.LEVEL_MEASURE, apply=False)[1][0]), b


def test_rows_pipeline_windows_device_output_and_f16_are_the_same_bits(pkg, model, ids, plain, desc, trimmed):
    fd = 60
    model.set_edges(**desc[fd])
    want = trimmed[fd]
    want_rows = np.stack([r for _, r in want])
    want_len = want_rows[:, 2]
    frames = plain[fd][2]
    # a row of the ragged batch equals its batch-1 call
    for b in range(3):
        one, l1, _ = model.process_batch(ids[b:b + 1, :LENS[b]], noise_seed=7, fixed_duration=fd, noise_seed_offsets=np.array([b], np.int32))
        assert l1[0] == want_len[b] and same(one[0], want[b][0]) and np.array_equal(model.last_edges()[0], want_rows[b]), b
    # vocoder windows without a sink: the stage runs behind the last window
    got, l2, _ = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=fd, vocoder_chunk_frames=257)
    assert np.array_equal(l2, want_len) and all(same(got[b], want[b][0]) for b in range(3)) and np.array_equal(model.last_edges(), want_rows)
    # submit / wait: the lengths and the rows of the batch that wait returned
    model.submit_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=fd)
    model.submit_batch(ids[:2], id_lengths=LENS[:2], noise_seed=7, fixed_duration=fd, vocoder_chunk_frames=257)
    got, l2, f2 = model.wait()
    assert np.array_equal(l2, want_len) and np.array_equal(f2, frames) and all(same(got[b], want[b][0]) for b in range(3))
    assert np.array_equal(model.last_edges(), want_rows)
    got, l2, _ = model.wait()
    assert np.array_equal(l2, want_len[:2]) and all(same(got[b], want[b][0]) for b in range(2)) and np.array_equal(model.last_edges(), want_rows[:2])
    # a caller-owned device buffer without a host copy: the stride check uses the bound, nothing behind a row's bound is written
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    bound = plain[fd][1] + PADS
    cap = int(bound.max()) + 3
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), 3 * cap * 4) == 0
    try:
        with pytest.raises(pkg.VitsError, match="out_device_stride"):
            model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=fd, out_device=dev.value, out_device_stride=int(bound.max()) - 1, skip_host_copy=True)
        assert hip.hipMemcpy(dev, np.full((3, cap), 7.25, np.float32).ctypes.data_as(C.c_void_p), 3 * cap * 4, 1) == 0
        none, l3, _ = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=fd, out_device=dev.value, out_device_stride=cap, skip_host_copy=True)
        got = np.zeros((3, cap), np.float32)
        assert hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), dev, got.nbytes, 2) == 0
        assert none is None and np.array_equal(l3, want_len) and all(same(got[b, :want_len[b]], want[b][0]) for b in range(3))
        for b in range(3):
            assert not got[b, want_len[b]:bound[b]].any() and (got[b, bound[b]:] == 7.25).all(), b
        assert np.array_equal(model.last_edges(), want_rows)
    finally:
        hip.hipFree(dev)
    # 16-bit arithmetic: the stage on that mode's own waveform
    model.set_arith(pkg.ARITH_F16)
    pcm, lengths, _ = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=fd, collect_taps=True)
    for b in range(3):
        y, n1, rows = pkg.edges(model.tap("waveform", b).ravel(), FS, **desc[fd])
        assert lengths[b] == n1[0] and same(pcm[b], y[0, :n1[0]]) and np.array_equal(model.last_edges()[b], rows[0]), b


def test_a_batch_split_inside_the_call_reports_every_row(pkg, tiny_bytes, ids, desc, trimmed, monkeypatch):
    monkeypatch.setenv("VITS_SPLIT_MIN_BATCH", "2")
    with pkg.Model(tiny_bytes) as m:
        m.set_edges(**desc[60])
        pcm, lengths, _ = m.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=60)
        want = trimmed[60]
        assert all(same(pcm[b], want[b][0]) and lengths[b] == want[b][1][2] for b in range(3))
        assert np.array_equal(m.last_edges(), np.stack([r for _, r in want]))


def test_voice_conversion_delivers_through_the_stage(pkg):
    rng = np.random.default_rng(5)
    lens = np.array([FS // 2, FS // 25 + 3], np.int64)
    x = np.full((2, int(lens.max()) + 2), np.nan, np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = 0.3 * rng.standard_normal(n).astype(np.float32)
    with pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_TINY | pkg.SYNTH_POSTERIOR)) as m:
        plain = m.convert_batch(x, lens, noise_seed=3)
        assert m.last_edges() is None
        th = choose(plain[0], need=0)  # (whether it trims these two is not the point here: the call goes through the stage)
        assert th is not None
        d = dict(SHAPE, mode=pkg.EDGES_TRIM_RELATIVE, threshold_db=th)
        m.set_edges(**d)
        got = m.convert_batch(x, lens, noise_seed=3)
        for b in range(2):
            assert ER.margin(plain[0][b], FS, ER.TRIM_RELATIVE, d["threshold_db"], **SHAPE) >= MARGIN
            y, n1, rows = pkg.edges(plain[0][b], FS, **d)
            assert got[1][b] == n1[0] and same(got[0][b], y[0, :n1[0]]) and np.array_equal(m.last_edges()[b], rows[0]), b
        with pytest.raises(pkg.VitsError, match="edges.*end"):
            m.convert_batch(x, lens, noise_seed=3, vocoder_chunk_frames=8, on_chunk=lambda u, off, p: False)


def test_nothing_changes_with_the_stage_off(pkg, tiny_bytes, ids, desc):
    out = {}
    for touched in (False, True):
        with pkg.Model(tiny_bytes) as m:
            assert m.edges["mode"] == pkg.EDGES_OFF
            if touched:
                m.set_edges(**desc[60])
                m.set_edges(pkg.EDGES_OFF)
                assert m.edges == dict(mode=0, threshold_db=0.0, keep_head_ms=0.0, keep_tail_ms=0.0, fade_in_ms=0.0, fade_out_ms=0.0, lead_ms=0.0, tail_ms=0.0)
            m.prof_enable(True)
            m.prof_reset()
            pcm, lengths, _ = m.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=60)
            assert '"edges_' not in json.dumps(m.prof_report()) and m.last_edges() is None
            m.prof_enable(False)
            out[touched] = (pcm, lengths, m.weight_bytes)
            if touched:
                # the first call that runs the stage allocates the rows (64 x (4 int64 + 1 int32)) and the fade tables (80 + 144 floats), once
                m.set_edges(**desc[60])
                assert m.weight_bytes == out[touched][2]
                m.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=60)
                w = m.weight_bytes
                assert w == out[touched][2] + 64 * 36 + (80 + 144) * 4
                m.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=60)
                assert m.weight_bytes == w
                # other fades: the tables are replaced, not added
                m.set_edges(pkg.EDGES_PAD, fade_in_ms=1.0)
                m.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=60)
                assert m.weight_bytes == out[touched][2] + 64 * 36 + 16 * 4
    assert all(same(out[False][0][b], out[True][0][b]) for b in range(3)) and np.array_equal(out[False][1], out[True][1]) and out[False][2] == out[True][2]


def test_refusals_leave_the_handle_as_it_was(pkg, model, ids, desc):
    model.set_edges(**desc[60])
    before = model.edges
    called = []
    with pytest.raises(pkg.VitsError, match="on_chunk.*edges.*the end of the utterance decides"):
        model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=3, vocoder_chunk_frames=13, on_chunk=lambda u, off, x: called.append(u) and False)
    assert not called
    with pytest.raises(pkg.VitsError, match="async.*edges.*host read"):
        model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=3, skip_host_copy=True, async_=True)
    # the desc
    for bad in (dict(mode=4), dict(mode=-1), dict(threshold_db=0.5), dict(threshold_db=float("nan")), dict(keep_head_ms=-1.0), dict(fade_out_ms=2000.5),
                dict(lead_ms=float("inf")), dict(tail_ms=float("nan"))):
        with pytest.raises(pkg.VitsError, match="vits_model_set_edges"):
            model.set_edges(**dict(desc[60], **bad))
        assert model.edges == before
    d = pkg.edges_desc(**desc[60])
    d.struct_size = 32
    assert pkg.lib().vits_model_set_edges(model._h, C.byref(d)) == -1 and "struct_size" in pkg.last_error() and model.edges == before
    # with a batch in flight
    model.submit_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=3)
    with pytest.raises(pkg.VitsError, match="batches in flight"):
        model.set_edges(pkg.EDGES_OFF)
    model.wait()
    assert model.edges == before
    # NULL switches it off; from inside on_chunk the handle is busy
    assert pkg.lib().vits_model_set_edges(model._h, None) == 0 and model.edges["mode"] == pkg.EDGES_OFF
    seen = []

    def sink(u, off, x):
        try:
            model.set_edges(**desc[60])
        except pkg.VitsError as e:
            seen.append(str(e))
        return False

    model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=3, vocoder_chunk_frames=8, on_chunk=sink)
    assert seen and all("model busy" in s for s in seen)
    assert model.edges["mode"] == pkg.EDGES_OFF
