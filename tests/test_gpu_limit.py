"""The loudness target under a ceiling through the engine (vits_model_set_limiter, limiter.hip): what a call reports and delivers is the operator's
limiting (vits_op_limit) of the model-rate waveform, bit for bit, through every way a call can deliver it (batch rows, the pipeline, vocoder windows, a
device buffer, another output rate, 16-bit arithmetic, voice conversion); the delivered loudness is closer to what was asked for than the ceiling rule's;
on_chunk is refused with the reason; nothing changes with the limiter off; the refusals.

The test's own values: one LEVEL_MEASURE call gives L and P of every utterance; the calls then ask for LEVEL_LOUDNESS at value_db = L of utterance 0
under ceiling_db = 20 log10(P of utterance 0) - 6: in range for a tanh output, and the ceiling binds by construction (g0 = 1, the peak 6 dB over)."""
import ctypes as C
import json

import numpy as np
import pytest

import limiter_ref as LR
import loudness_ref as R

pytestmark = pytest.mark.gpu

FS = 16000
LENS = np.array([5, 12, 31], np.int32)
FD = 200  # frames per token: 0.5 s, 1.2 s and 3.1 s at hop 8, every utterance measurable
L_TOL = 0.01  # LU, as tests/test_gpu_level.py


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
        assert m.sampling_rate == FS and m.hop == 8
        yield m


@pytest.fixture(scope="module")
def measured(pkg, tiny, ids):
    """(waveforms, lengths, frames, levels of LEVEL_MEASURE, value_db, ceiling_db)"""
    tiny.set_limiter(pkg.LIMIT_OFF)
    tiny.set_level(pkg.LEVEL_MEASURE)
    pcm, lengths, frames = tiny.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=FD)
    levels = tiny.last_levels()
    assert tiny.last_limits() is None
    tiny.set_level(pkg.LEVEL_NONE)
    assert (levels[:, 3] > 0).all()
    value, ceiling = float(levels[0, 0]), float(np.float32(20.0 * np.log10(float(levels[0, 1])) - 6.0))
    print(f"measured: L = {levels[:, 0].tolist()} LUFS, P = {levels[:, 1].tolist()}; the calls ask for {value:.3f} LUFS under {ceiling:.3f} dB")
    assert -70 <= value <= 0 and -60 <= ceiling <= 0
    return pcm, lengths, frames, levels, value, ceiling


@pytest.fixture()
def model(pkg, tiny):
    """the shared handle; without limiter and level, at the model's rate and fp32 afterwards"""
    yield tiny
    tiny.set_arith(pkg.ARITH_F32)
    tiny.set_rates(0, 0)
    tiny.set_level(pkg.LEVEL_NONE)
    tiny.set_limiter(pkg.LIMIT_OFF)


def op(pkg, wave, kind, value, ceiling):
    """the operator on one waveform: (y [N], levels [4], limits [4])"""
    y, levels, limits = pkg.limit(wave, FS, kind, value, ceiling)
    return y[0, :wave.size], levels[0], limits[0]


@pytest.fixture(scope="module")
def limited(pkg, tiny, ids, measured):
    """the anchor of the tests below: the operator on the measured call's waveforms, computed once"""
    _, _, _, _, value, ceiling = measured
    return [op(pkg, w, pkg.LEVEL_LOUDNESS, value, ceiling) for w in measured[0]]


def test_a_call_reports_and_delivers_the_operators_limiting(pkg, model, ids, measured, limited):
    waves, lengths0, frames0, lv0, value, ceiling = measured
    model.set_limiter(pkg.LIMIT_TRUE_PEAK)
    assert model.limiter == pkg.LIMIT_TRUE_PEAK
    model.set_level(pkg.LEVEL_LOUDNESS, value, ceiling)
    pcm, lengths, frames = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=FD, collect_taps=True)
    levels, limits = model.last_levels(), model.last_limits()
    assert levels.shape == limits.shape == (3, 4) and np.array_equal(lengths, lengths0) and np.array_equal(frames, frames0)
    c = 10.0 ** (ceiling / 20.0)
    for b in range(3):
        wave = model.tap("waveform", b).ravel()
        assert same(wave, waves[b])  # (the model-rate waveform is what it was)
        y, row, lim = limited[b]
        assert same(pcm[b], y) and same(levels[b], row) and same(limits[b], lim), b
        assert same(model.tap("waveform_level", b).ravel(), y), b
        assert same(levels[b, :2], lv0[b, :2]) and levels[b, 3] == lv0[b, 3]
        assert abs(20 * np.log10(float(levels[b, 2])) - (value - float(levels[b, 0]))) <= 1e-4  # g = g0: the ceiling no longer reduces it
        assert np.abs(pcm[b]).max() <= c * (1 + 2.0 ** -22)
    assert levels[0, 2] == 1.0 and limits[0, 2] < 0.75 and limits[0, 3] > 0  # utterance 0: its peak is 6 dB over, by construction
    print("limits:", limits.tolist())
    # the limiter off: the same settings deliver today's bits, the ceiling rule's
    model.set_limiter(pkg.LIMIT_OFF)
    rule, _, _ = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=FD)
    assert model.last_limits() is None
    for b in range(3):
        yl, ll = pkg.level(waves[b], FS, pkg.LEVEL_LOUDNESS, value, ceiling)
        assert same(rule[b], yl[0, :waves[b].size]) and same(model.last_levels()[b], ll[0]), b
    # what was asked for: the delivered loudness is strictly closer to value_db than the ceiling rule's, and it is the restatement's
    for b in range(3):
        got, by_rule = pkg.loudness_host(pcm[b], FS)[0], pkg.loudness_host(rule[b], FS)[0]
        u = pkg.resample(waves[b], FS, 4 * FS)[0][0]
        want = R.loudness(LR.limiter(waves[b], FS, float(levels[b, 2]), float(np.float32(c)), u=u)["y"].astype(np.float32), FS)[0]
        print(f"utterance {b}: asked {value:.3f} LUFS, limiter {got:.3f}, ceiling rule {by_rule:.3f}, restatement {want:.3f}")
        assert abs(got - want) <= L_TOL, b
        if float(levels[b, 2]) * float(limits[b, 0]) > c:  # (the ceiling binds on this utterance)
            assert abs(got - value) < abs(by_rule - value), b
    assert float(levels[0, 2]) * float(limits[0, 0]) > c


def test_rows_pipeline_windows_and_device_output_are_the_same_bits(pkg, model, ids, measured, limited):
    _, lengths, frames, _, value, ceiling = measured
    model.set_limiter(pkg.LIMIT_TRUE_PEAK)
    model.set_level(pkg.LEVEL_LOUDNESS, value, ceiling)
    want_lv, want_lm = np.stack([r[1] for r in limited]), np.stack([r[2] for r in limited])
    pcm = [r[0] for r in limited]
    # a row of the ragged batch equals its batch-1 call
    for b in range(3):
        one, l1, _ = model.process_batch(ids[b:b + 1, :LENS[b]], noise_seed=7, fixed_duration=FD, noise_seed_offsets=np.array([b], np.int32))
        assert l1[0] == lengths[b] and same(one[0], pcm[b]) and same(model.last_levels()[0], want_lv[b]) and same(model.last_limits()[0], want_lm[b]), b
    # vocoder windows without a sink: the limiter runs behind the last window
    got, l2, _ = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=FD, vocoder_chunk_frames=257)
    assert np.array_equal(l2, lengths) and all(same(got[b], pcm[b]) for b in range(3)) and same(model.last_limits(), want_lm) and same(model.last_levels(), want_lv)
    # submit / wait: the rows of the batch that wait returned
    model.submit_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=FD)
    model.submit_batch(ids[:2], id_lengths=LENS[:2], noise_seed=7, fixed_duration=FD, vocoder_chunk_frames=257)
    got, l2, f2 = model.wait()
    assert np.array_equal(l2, lengths) and np.array_equal(f2, frames) and all(same(got[b], pcm[b]) for b in range(3))
    assert same(model.last_limits(), want_lm) and same(model.last_levels(), want_lv)
    got, l2, _ = model.wait()
    assert all(same(got[b], pcm[b]) for b in range(2)) and same(model.last_limits(), want_lm[:2])
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
            none, l3, _ = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=FD, out_device=dev.value, out_device_stride=cap,
                                              skip_host_copy=True, async_=async_)
            if async_:
                model.sync()
            got = np.zeros((3, cap), np.float32)
            assert hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), dev, got.nbytes, 2) == 0
            assert none is None and np.array_equal(l3, lengths) and all(same(got[b, :lengths[b]], pcm[b]) for b in range(3)), async_
            assert not got[0, lengths[0]:].any()  # nothing written behind an utterance
            assert same(model.last_limits(), want_lm) and same(model.last_levels(), want_lv), async_
    finally:
        hip.hipFree(dev)


def test_a_batch_split_inside_the_call_reports_every_row(pkg, tiny_bytes, ids, measured, limited, monkeypatch):
    _, _, _, _, value, ceiling = measured
    monkeypatch.setenv("VITS_SPLIT_MIN_BATCH", "2")
    with pkg.Model(tiny_bytes) as m:
        m.set_limiter(pkg.LIMIT_TRUE_PEAK)
        m.set_level(pkg.LEVEL_LOUDNESS, value, ceiling)
        pcm, _, _ = m.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=FD)
        assert all(same(pcm[b], limited[b][0]) for b in range(3))
        assert same(m.last_limits(), np.stack([r[2] for r in limited])) and same(m.last_levels(), np.stack([r[1] for r in limited]))


def test_the_limiter_comes_before_the_resampler(pkg, model, ids, measured, limited):
    _, _, _, _, value, ceiling = measured
    model.set_limiter(pkg.LIMIT_TRUE_PEAK)
    model.set_level(pkg.LEVEL_LOUDNESS, value, ceiling)
    model.set_rates(output_rate=44100)
    pcm, lengths, _ = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=FD, collect_taps=True)
    for b in range(3):
        y = limited[b][0]
        assert same(model.tap("waveform_level", b).ravel(), y) and same(model.last_limits()[b], limited[b][2])
        out, n = pkg.resample(y, FS, 44100)
        assert lengths[b] == n[0] and same(pcm[b], out[0, :n[0]]), b


def test_gain_and_true_peak_normalisation(pkg, model, ids, measured):
    waves = measured[0]
    model.set_limiter(pkg.LIMIT_TRUE_PEAK)
    for kind, value, ceiling in ((pkg.LEVEL_GAIN, 9.0, -3.0), (pkg.LEVEL_PEAK, -2.0, 0.0)):
        model.set_level(kind, value, ceiling)
        assert model.level == (kind, value, ceiling)  # (with the limiter on a gain keeps its ceiling)
        pcm, _, _ = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=FD)
        for b in range(3):
            y, row, lim = op(pkg, waves[b], kind, value, ceiling)
            assert same(pcm[b], y) and same(model.last_levels()[b], row) and same(model.last_limits()[b], lim), (kind, b)
        if kind == pkg.LEVEL_PEAK:
            assert (np.abs(20 * np.log10(model.last_limits()[:, 1].astype(np.float64)) + 2.0) <= 1e-3).all()
    # under NONE and MEASURE nothing is queued
    model.set_level(pkg.LEVEL_MEASURE)
    pcm, _, _ = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=FD)
    assert model.last_limits() is None and all(same(pcm[b], waves[b]) for b in range(3))


def test_f16_arithmetic_limits_its_own_waveform(pkg, model, ids, measured):
    _, _, _, _, value, ceiling = measured
    model.set_arith(pkg.ARITH_F16)
    model.set_limiter(pkg.LIMIT_TRUE_PEAK)
    model.set_level(pkg.LEVEL_LOUDNESS, value, ceiling)
    pcm, _, _ = model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=FD, collect_taps=True)
    for b in range(3):
        y, row, lim = op(pkg, model.tap("waveform", b).ravel(), pkg.LEVEL_LOUDNESS, value, ceiling)
        assert same(pcm[b], y) and same(model.last_levels()[b], row) and same(model.last_limits()[b], lim), b


def test_voice_conversion_delivers_the_operators_limiting(pkg):
    rng = np.random.default_rng(5)
    lens = np.array([FS // 2, FS // 25 + 3], np.int64)
    x = np.full((2, int(lens.max()) + 2), np.nan, np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = 0.3 * rng.standard_normal(n).astype(np.float32)
    with pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_TINY | pkg.SYNTH_POSTERIOR)) as m:
        plain = m.convert_batch(x, lens, noise_seed=3)
        peak = max(float(np.abs(p).max()) for p in plain[0])
        ceiling = float(np.float32(20 * np.log10(peak) - 6.0))
        m.set_limiter(pkg.LIMIT_TRUE_PEAK)
        m.set_level(pkg.LEVEL_GAIN, 0.0, ceiling)
        got = m.convert_batch(x, lens, noise_seed=3)
        for b in range(2):
            y, row, lim = op(pkg, plain[0][b], pkg.LEVEL_GAIN, 0.0, ceiling)
            assert same(got[0][b], y) and same(m.last_levels()[b], row) and same(m.last_limits()[b], lim), b
        assert m.last_limits()[:, 2].min() < 0.75


def test_on_chunk_refuses_and_says_why(pkg, model, ids):
    model.set_limiter(pkg.LIMIT_TRUE_PEAK)
    model.set_level(pkg.LEVEL_GAIN, -2.0, -1.0)
    called = []
    with pytest.raises(pkg.VitsError, match="limiter.*looks 80 samples ahead and 880 back.*halo"):
        model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=3, vocoder_chunk_frames=13, on_chunk=lambda u, off, x: called.append(u) and False)
    assert not called
    # (with the limiter off the gain streams as it did)
    model.set_limiter(pkg.LIMIT_OFF)
    model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=3, vocoder_chunk_frames=13, on_chunk=lambda u, off, x: called.append(u) and False)
    assert called


def test_nothing_changes_with_the_limiter_off(pkg, tiny_bytes, ids, measured):
    _, _, _, _, value, ceiling = measured
    out = {}
    for touched in (False, True):
        with pkg.Model(tiny_bytes) as m:
            assert m.limiter == pkg.LIMIT_OFF
            if touched:
                m.set_limiter(pkg.LIMIT_TRUE_PEAK)
                m.set_limiter(pkg.LIMIT_OFF)
            m.set_level(pkg.LEVEL_LOUDNESS, value, ceiling)
            m.prof_enable(True)
            m.prof_reset()
            pcm, _, _ = m.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=FD)
            assert '"limit"' not in json.dumps(m.prof_report()) and m.last_limits() is None
            m.prof_enable(False)
            out[touched] = (pcm, m.last_levels(), m.weight_bytes)
            if touched:
                # the first call that limits allocates the limits rows and the 4x table, once
                m.set_limiter(pkg.LIMIT_TRUE_PEAK)
                assert m.weight_bytes == out[touched][2]
                m.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=FD)
                w = m.weight_bytes
                assert w == out[touched][2] + 64 * 4 * 4 + 4 * 71 * 4
                m.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=FD)
                assert m.weight_bytes == w
    assert all(same(out[False][0][b], out[True][0][b]) for b in range(3)) and same(out[False][1], out[True][1]) and out[False][2] == out[True][2]


def test_refusals_leave_the_mode_as_it_was(pkg, model, ids):
    model.set_limiter(pkg.LIMIT_TRUE_PEAK)
    for bad in (2, -1, 7):
        with pytest.raises(pkg.VitsError, match="vits_model_set_limiter.*unknown mode"):
            model.set_limiter(bad)
        assert model.limiter == pkg.LIMIT_TRUE_PEAK
    # with the limiter on a gain's ceiling is checked too
    model.set_level(pkg.LEVEL_GAIN, 3.0, -1.5)
    for bad in (0.5, -61.0, float("nan")):
        with pytest.raises(pkg.VitsError, match="vits_model_set_level.*ceiling_db"):
            model.set_level(pkg.LEVEL_GAIN, 3.0, bad)
        assert model.level == (pkg.LEVEL_GAIN, 3.0, -1.5)
    # with a batch in flight
    model.submit_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=3)
    with pytest.raises(pkg.VitsError, match="batches in flight"):
        model.set_limiter(pkg.LIMIT_OFF)
    model.wait()
    assert model.limiter == pkg.LIMIT_TRUE_PEAK
    # from inside on_chunk
    model.set_limiter(pkg.LIMIT_OFF)
    seen = []

    def sink(u, off, x):
        try:
            model.set_limiter(pkg.LIMIT_TRUE_PEAK)
        except pkg.VitsError as e:
            seen.append(str(e))
        return False

    model.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=3, vocoder_chunk_frames=8, on_chunk=sink)
    assert seen and all("model busy" in s for s in seen)
    assert model.limiter == pkg.LIMIT_OFF
