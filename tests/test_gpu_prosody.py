"""Per-utterance prosody on the GPU: speaking rate, noise scales, duration overrides and durations_out. Against transformers taps
(tests/golden/make_golden_prosody.py), against model files that hold each value (bit for bit, at the same batch shape: plain, f16, in-call
split, submit / wait, windowed, frames-only), the model-level values (vits_model_set_prosody, the reference entry points), overrides, the
emulated-ggml exact stage one against the oracle, and every refusal."""
import numpy as np
import pytest

from conftest import golden, rel_err
from test_prosody_host import FIXTURES, fixture_bytes, with_prosody

pytestmark = pytest.mark.gpu

FILE = (1.0, 0.667, 0.8)  # the synthetic model's own values (model_file.cpp)
TRIPLES = [FILE, (0.6, 1.0, 0.0), (1.7, 0.3, 1.2)]
PICK = np.array([1, 0, 2, 2, 1, 0], np.int32)  # the triple of each utterance of the mixed batch
LENS = np.array([40, 7, 33, 40, 1, 20], np.int32)


def arrays(pick):
    t = np.array(TRIPLES, np.float32)[pick]
    return dict(speaking_rate=t[:, 0].copy(), noise_scale=t[:, 1].copy(), noise_scale_duration=t[:, 2].copy())


@pytest.fixture(scope="module")
def ids(pkg):
    return pkg.synth_ids(6, 40, ids_seed=77)


@pytest.fixture(scope="module")
def full(pkg, full_bytes):
    m = pkg.Model(full_bytes)
    yield m
    m.close()


@pytest.mark.parametrize("fixture,mode", FIXTURES)
def test_prosody_matches_transformers_taps(pkg, fixture, mode):
    """Every setting of the fixture in ONE batch, as per-utterance arrays: durations exact, log_duration / z_flow / waveform within 2e-4."""
    g = golden(fixture)
    dec = int(g["decimate"][0])
    s = g["settings"]
    n = s.shape[0]
    ids = np.repeat(g["ids"][None], n, axis=0)
    with pkg.Model(fixture_bytes(pkg, fixture)) as m:
        dout = np.zeros(ids.shape, np.int32)
        pcm, lengths, frames = m.process_batch(ids, mode=mode, noise_kind=pkg.NOISE_EXPLICIT, noise_dur=np.repeat(g["noise_dur"][None], n, axis=0),
                                               noise_prior=np.repeat(g["noise_prior"][None], n, axis=0), collect_taps=True, speaking_rate=s[:, 0],
                                               noise_scale=s[:, 1], noise_scale_duration=s[:, 2], durations_out=dout)
        for i in range(n):
            k = "p%d_" % i
            np.testing.assert_array_equal(m.tap("durations", i), g[k + "durations"].ravel(), err_msg=k)
            np.testing.assert_array_equal(dout[i], g[k + "durations"].ravel().astype(np.int32), err_msg=k)
            assert frames[i] == int(g[k + "durations"].sum())
            assert rel_err(m.tap("log_duration", i), g[k + "log_duration"]) < 2e-4, k
            assert rel_err(m.tap("z_flow", i), g[k + "z_flow"]) < 2e-4, k
            assert lengths[i] == int(g[k + "waveform_len"][0]), k
            assert rel_err(pcm[i][::dec], g[k + "waveform"]) < 2e-4, k


def _run(m, ids, variant, **kw):
    """(pcm list or None, lengths, frames, durations_out) of one call in the given variant"""
    dout = np.zeros(ids.shape, np.int32)
    if variant == "submit":
        m.submit_batch(ids, id_lengths=LENS, noise_seed=5, durations_out=dout, **kw)
        pcm, lengths, frames = m.wait()
    else:
        extra = {"plain": {}, "split": {}, "chunked": dict(vocoder_chunk_frames=24), "frames_only": dict(frames_only=True)}[variant]
        pcm, lengths, frames = m.process_batch(ids, id_lengths=LENS, noise_seed=5, durations_out=dout, **extra, **kw)
    return pcm, lengths, frames, dout


@pytest.mark.parametrize("arith", ["f32", "f16"])
@pytest.mark.parametrize("variant", ["plain", "split", "submit", "chunked", "frames_only"])
def test_mixed_batch_rows_equal_a_file_that_holds_the_value(pkg, full_bytes, ids, monkeypatch, arith, variant):
    """For each triple v of a mixed batch: the rows whose value is v equal, bit for bit, the same rows of the same batch run without arrays on a
    model file that holds v (same shape, so the same kernel choices): PCM, lengths, frames and durations_out."""
    monkeypatch.setenv("VITS_SPLIT_MIN_BATCH", "2" if variant == "split" else "0")
    a = pkg.ARITH_F32 if arith == "f32" else pkg.ARITH_F16
    with pkg.Model(full_bytes) as m:
        m.set_arith(a)
        got = _run(m, ids, variant, **arrays(PICK))
    for v, triple in enumerate(TRIPLES):
        with pkg.Model(with_prosody(full_bytes, *triple)) as mv:
            mv.set_arith(a)
            want = _run(mv, ids, variant)
        rows = np.flatnonzero(PICK == v)
        np.testing.assert_array_equal(got[1][rows], want[1][rows])
        np.testing.assert_array_equal(got[2][rows], want[2][rows])
        np.testing.assert_array_equal(got[3][rows], want[3][rows])
        if variant != "frames_only":
            for b in rows:
                assert np.array_equal(got[0][b], want[0][b]), (variant, arith, v, b)
    assert len(set(got[2].tolist())) > 2


def test_model_values_as_arrays_and_set_prosody_to_the_file_values_change_nothing(pkg, full, ids):
    want = full.process_batch(ids, id_lengths=LENS, noise_seed=11)
    assert full.get_prosody() == tuple(float(np.float32(x)) for x in FILE)
    got = full.process_batch(ids, id_lengths=LENS, noise_seed=11, **arrays(np.zeros(6, np.int32)))
    full.set_prosody(*FILE)
    again = full.process_batch(ids, id_lengths=LENS, noise_seed=11)
    for r in (got, again):
        np.testing.assert_array_equal(r[1], want[1])
        np.testing.assert_array_equal(r[2], want[2])
        for b in range(6):
            assert np.array_equal(r[0][b], want[0][b]), b
    # the attribute form, as transformers users write it
    full.speaking_rate = 1.5
    assert full.speaking_rate == 1.5 and full.get_prosody()[1:] == tuple(float(np.float32(x)) for x in FILE[1:])
    full.speaking_rate = FILE[0]


def test_zero_noise_scales_remove_the_noise(pkg, full, ids):
    a = full.process_batch(ids, id_lengths=LENS, noise_seed=1, noise_scale=0.0, noise_scale_duration=0.0)
    b = full.process_batch(ids, id_lengths=LENS, noise_seed=987654, noise_scale=0.0, noise_scale_duration=0.0)
    np.testing.assert_array_equal(a[2], b[2])
    for u in range(6):
        assert np.array_equal(a[0][u], b[0][u]), u
    c = full.process_batch(ids, id_lengths=LENS, noise_seed=987654)
    assert any(c[0][u].size != a[0][u].size or not np.array_equal(c[0][u], a[0][u]) for u in range(6))


@pytest.mark.parametrize("rate", [0.25, 1.7])
def test_set_prosody_drives_the_reference_entry_point(pkg, full_bytes, ids, rate):
    """vits_model_process_ids (reference noise stream, the look-ahead of the prior draw sized by the length scale; 0.25 stretches past the
    default block) after set_prosody == the same call on a file that holds the values."""
    one = ids[0, :LENS[0]]
    with pkg.Model(with_prosody(full_bytes, rate, 0.5, 0.9)) as mf:
        pkg.lib().vits_reference_noise_seed(3)
        want = mf.process_ids(one)
        want2 = mf.process_ids(one)
    with pkg.Model(full_bytes) as m:
        explicit = m.process_batch(ids, id_lengths=LENS, noise_seed=2, **arrays(PICK))
        m.set_prosody(rate, 0.5, 0.9)
        assert m.get_prosody() == (float(np.float32(rate)), 0.5, float(np.float32(0.9)))
        pkg.lib().vits_reference_noise_seed(3)
        got = m.process_ids(one)
        got2 = m.process_ids(one)
        again = m.process_batch(ids, id_lengths=LENS, noise_seed=2, **arrays(PICK))  # explicit arrays: the model values do not matter
    assert np.array_equal(got, want) and np.array_equal(got2, want2)
    np.testing.assert_array_equal(again[2], explicit[2])
    for b in range(6):
        assert np.array_equal(again[0][b], explicit[0][b]), b


def test_duration_overrides(pkg, full, ids):
    base_out = np.zeros(ids.shape, np.int32)
    base = full.process_batch(ids, id_lengths=LENS, noise_seed=4, durations_out=base_out, speaking_rate=0.8)

    def same(r, want=base):
        np.testing.assert_array_equal(r[1], want[1])
        np.testing.assert_array_equal(r[2], want[2])
        for b in range(6):
            assert np.array_equal(r[0][b], want[0][b]), b

    # all -1: the prediction
    same(full.process_batch(ids, id_lengths=LENS, noise_seed=4, speaking_rate=0.8, duration_override=np.full(ids.shape, -1, np.int32)))
    # a previous call's durations_out: that call
    same(full.process_batch(ids, id_lengths=LENS, noise_seed=4, speaking_rate=0.8, duration_override=base_out))
    # every token d: fixed_duration = d
    for d in (1, 3):
        fixed = full.process_batch(ids, id_lengths=LENS, noise_seed=4, fixed_duration=d)
        same(full.process_batch(ids, id_lengths=LENS, noise_seed=4, duration_override=np.full(ids.shape, d, np.int32)), fixed)
    # mixed: the override where one is given (0 included), the prediction elsewhere; frames = the sum
    ovr = np.full(ids.shape, -1, np.int32)
    ovr[:, ::3] = 7
    ovr[:, 1::5] = 0
    out = np.zeros(ids.shape, np.int32)
    _, _, frames = full.process_batch(ids, id_lengths=LENS, noise_seed=4, speaking_rate=0.8, duration_override=ovr, durations_out=out)
    for b in range(6):
        n = LENS[b]
        np.testing.assert_array_equal(out[b, :n], np.where(ovr[b, :n] >= 0, ovr[b, :n], base_out[b, :n]))
        assert not out[b, n:].any()
        assert frames[b] == max(1, int(out[b].sum()))


def test_durations_out_equals_the_tap_and_arrives_early(pkg, full, ids):
    out = np.full(ids.shape, -5, np.int32)
    _, _, frames = full.process_batch(ids, id_lengths=LENS, noise_seed=6, collect_taps=True, durations_out=out, speaking_rate=PICK + 0.5)
    for b in range(6):
        np.testing.assert_array_equal(out[b, :LENS[b]], full.tap("durations", b).astype(np.int32))
        assert not out[b, LENS[b]:].any()
        assert frames[b] == max(1, int(out[b].sum()))
    # streaming: the timings are there before the first chunk of audio
    out2 = np.full(ids.shape, -5, np.int32)
    seen = []

    def sink(utt, off, pcm):
        seen.append(out2.copy())
        return False

    full.process_batch(ids, id_lengths=LENS, noise_seed=6, durations_out=out2, speaking_rate=PICK + 0.5, vocoder_chunk_frames=16, on_chunk=sink)
    assert seen and np.array_equal(seen[0], out)
    # pipelined: filled by the matching wait at the latest
    o1, o2 = np.full(ids.shape, -5, np.int32), np.full(ids.shape, -5, np.int32)
    full.submit_batch(ids, id_lengths=LENS, noise_seed=6, durations_out=o1, speaking_rate=PICK + 0.5)
    full.submit_batch(ids, id_lengths=LENS, noise_seed=6, durations_out=o2)
    full.wait()
    np.testing.assert_array_equal(o1, out)
    full.wait()
    ref = np.zeros(ids.shape, np.int32)
    full.process_batch(ids, id_lengths=LENS, noise_seed=6, durations_out=ref, frames_only=True)
    np.testing.assert_array_equal(o2, ref)
    # fixed_duration: every token, on the host
    fx = np.full(ids.shape, -5, np.int32)
    full.process_batch(ids, id_lengths=LENS, noise_seed=6, durations_out=fx, fixed_duration=2, noise_scale=0.1)
    for b in range(6):
        assert (fx[b, :LENS[b]] == 2).all() and not fx[b, LENS[b]:].any()


@pytest.mark.parametrize("mode", [0, 1])
def test_emulated_tables_mode_one_durations_equal_the_oracle_on_rewritten_files(pkg, oracle, full, full_bytes, ids, mode):
    rates = np.array([0.6, 1.0, 1.7, 2.5, 0.6, 1.3], np.float32)
    full.set_ggml_tables(1)
    try:
        out = np.zeros(ids.shape, np.int32)
        _, _, frames = full.process_batch(ids, id_lengths=LENS, mode=mode, noise_seed=4321, frames_only=True, durations_out=out, speaking_rate=rates,
                                          noise_scale_duration=np.float32(0.5))
    finally:
        full.set_ggml_tables(0)
    for b in range(6):
        om = oracle.Model(with_prosody(full_bytes, rates[b], FILE[1], 0.5))
        _, dur = om.log_durations(ids[b, :LENS[b]], mode=mode, noise_seed=4321 + b, ggml_tables=1)
        np.testing.assert_array_equal(out[b, :LENS[b]], dur.astype(np.int32), err_msg="utterance %d" % b)
        assert frames[b] == max(1, int(dur.sum()))
        om.close()


def test_refusals_name_the_utterance_and_leave_the_handle_usable(pkg, full, ids):
    cases = [
        (dict(speaking_rate=np.array([1, 1, 0.05, 1, 1, 1], np.float32)), r"speaking_rates\[2\]"),
        (dict(speaking_rate=np.array([1, 1, 1, 1, np.nan, 1], np.float32)), r"speaking_rates\[4\]"),
        (dict(speaking_rate=np.array([11, 1, 1, 1, 1, 1], np.float32)), r"speaking_rates\[0\]"),
        (dict(noise_scale=np.array([0, 0, 0, -0.5, 0, 0], np.float32)), r"noise_scales\[3\]"),
        (dict(noise_scale_duration=np.array([0, np.inf, 0, 0, 0, 0], np.float32)), r"noise_scale_durations\[1\]"),
        (dict(noise_scale=np.array([0, 0, 0, 0, 0, 10.5], np.float32)), r"noise_scales\[5\]"),
    ]
    ovr = np.full(ids.shape, -1, np.int32)
    ovr[3, 5] = -2
    cases.append((dict(duration_override=ovr), r"utterance 3, token 5"))
    ovr2 = np.full(ids.shape, -1, np.int32)
    ovr2[0, 39] = 10001
    cases.append((dict(duration_override=ovr2), r"utterance 0, token 39"))
    cases.append((dict(speaking_rate=1.0, fixed_duration=2), "fixed_duration"))
    cases.append((dict(duration_override=np.zeros(ids.shape, np.int32), fixed_duration=2), "fixed_duration"))
    for kw, msg in cases:
        with pytest.raises(pkg.VitsError, match=msg):
            full.process_batch(ids, id_lengths=LENS, **kw)
        with pytest.raises(pkg.VitsError, match=msg):
            full.submit_batch(ids, id_lengths=LENS, **kw)
        assert full.pending == 0
    ovr3 = np.full(ids.shape, -1, np.int32)
    ovr3[1, 20] = 99999  # past id_lengths[1] = 7: never read, not refused
    full.process_batch(ids, id_lengths=LENS, duration_override=ovr3, frames_only=True)
    before = full.get_prosody()
    for bad in ((0.09, 0.5, 0.5), (1.0, -1.0, 0.5), (1.0, 0.5, float("nan")), (float("inf"), 0.5, 0.5)):
        with pytest.raises(pkg.VitsError, match="set_prosody"):
            full.set_prosody(*bad)
        assert full.get_prosody() == before
    with pytest.raises(pkg.VitsError, match="speaking_rate"):
        full.speaking_rate = 20.0
    # conversion takes none of the five
    with pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_TINY | pkg.SYNTH_SPEAKERS | pkg.SYNTH_POSTERIOR)) as vc:
        pcm = np.sin(np.arange(2048, dtype=np.float32) * 0.05)[None]
        for kw, field in ((dict(speaking_rate=[1.0]), "speaking_rates"), (dict(noise_scale=[0.5]), "noise_scales"),
                          (dict(noise_scale_duration=[0.5]), "noise_scale_durations"), (dict(duration_override=[-1]), "duration_override"),
                          (dict(durations_out=np.zeros(1, np.int32)), "durations_out")):
            with pytest.raises(pkg.VitsError, match=field):
                vc.convert_batch(pcm, src=0, tgt=1, **kw)
        vc.convert_batch(pcm, src=0, tgt=1)
    # the handle still works
    r = full.process_batch(ids, id_lengths=LENS, noise_seed=5)
    assert r[0] is not None and full.pending == 0
