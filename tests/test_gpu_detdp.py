"""Models with the deterministic duration predictor (use_stochastic_duration_prediction = False) on the GPU: against transformers taps
(tests/golden/make_golden_detdp.py), what "no noise is drawn" means for every noise kind, the bit identities (batch row / pipeline / fused against un-fused /
speakers and voices), prosody, the ggml-tables modes, and conversion / alignment on such a model."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden, rel_err
from test_speakers import read_file, write_file

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def export_bytes():
    with open(os.path.join(GOLDEN, "tiny_detdp_hf_export.ggml"), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def full_det_bytes(pkg):
    return pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL | pkg.SYNTH_SPEAKERS | pkg.SYNTH_DETERMINISTIC)


@pytest.fixture(scope="module")
def full_det(pkg, full_det_bytes):
    m = pkg.Model(full_det_bytes)
    yield m
    m.close()


def key(s):
    return "sm1" if s < 0 else "s%d" % s


@pytest.mark.parametrize("fixture,mode", [("tiny_detdp_hf_export_taps.npz", 1), ("tiny_detdp_hf_export_refmode_taps.npz", 0),
                                          ("full_synth_detdp_taps.npz", 1), ("full_synth_detdp_refmode_taps.npz", 0)])
def test_durations_and_audio_match_transformers(pkg, export_bytes, full_det_bytes, fixture, mode):
    """durations exact (the generator keeps every exp(logw) 1e-3 away from an integer); log_duration within 4 x the fixture's own |fp32 - float64|; z_flow and the
    waveform within the bounds tests/test_gpu_speakers.py applies to the same taps (the kernels behind the durations are unchanged)"""
    g = golden(fixture)
    dec = int(g["decimate"][0])
    with pkg.Model(export_bytes if fixture.startswith("tiny") else full_det_bytes) as m:
        assert m.duration_predictor_kind == pkg.DP_DETERMINISTIC
        for s in g["speakers"].tolist():
            k = key(s)
            # no noise_dur: VITS_NOISE_EXPLICIT must not demand it of such a model
            pcm, lengths, _ = m.process_batch(g["ids"], mode=mode, noise_kind=pkg.NOISE_EXPLICIT, noise_prior=g[k + "_noise_prior"][None], collect_taps=True, speaker_ids=[s])
            np.testing.assert_array_equal(m.tap("durations"), g[k + "_durations"].ravel(), err_msg=k)
            f64 = g[k + "_log_duration_f64"].astype(np.float64).ravel()
            bound = 4 * np.abs(g[k + "_log_duration"].astype(np.float64).ravel() - f64).max()
            err = np.abs(m.tap("log_duration").astype(np.float64) - f64).max()
            print("%s %s: |log_duration - f64| = %.3e, bound %.3e" % (fixture, k, err, bound))
            assert err <= bound, (k, err, bound)
            assert rel_err(m.tap("z_flow"), g[k + "_z_flow"]) < 2e-4, k
            assert lengths[0] == int(g[k + "_waveform_len"][0]), k
            assert rel_err(pcm[0][::dec], g[k + "_waveform"]) < 2e-4, k
            with pytest.raises(pkg.VitsError):
                m.tap("noise_dur")
        frames = {s: int(g[key(s) + "_durations"].sum()) for s in g["speakers"].tolist()}
        assert len(set(frames.values())) > 1  # the fixture's speakers really move the durations


def test_predictor_kind(pkg, full_det, tiny_bytes):
    assert full_det.duration_predictor_kind == 1
    with pkg.Model(tiny_bytes) as m:
        assert m.duration_predictor_kind == 0
    assert pkg.lib().vits_model_duration_predictor_kind(None) == -1


def test_the_reference_stream_is_not_advanced_for_a_duration_draw(pkg, oracle, full_det):
    ids = pkg.synth_ids(1, 12)
    pkg.lib().vits_reference_noise_seed(7)
    _, _, frames = full_det.process_batch(ids, noise_kind=pkg.NOISE_REFERENCE, collect_taps=True)
    F = 192
    got = full_det.tap("noise_prior")
    assert got.size == F * int(frames[0])
    # tensor_randn{L, F} in memory order [F][L] (vits.cpp:1059): the first F * L values of the stream seeded 7 — nothing was consumed in front of them
    np.testing.assert_array_equal(got, oracle.reference_noise(got.size, seed=7))


def test_noise_scale_duration_has_no_effect(pkg, full_det):
    ids = pkg.synth_ids(2, 20)
    a, _, fa = full_det.process_batch(ids, noise_seed=5, noise_scale_duration=[0.0, 0.3], speaker_ids=[4, -1])
    b, _, fb = full_det.process_batch(ids, noise_seed=5, noise_scale_duration=[1.5, 1.0], speaker_ids=[4, -1])
    np.testing.assert_array_equal(fa, fb)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    with pytest.raises(pkg.VitsError):  # validated as before
        full_det.process_batch(ids, noise_scale_duration=[0.5, 11.0])


LENS = np.array([48, 7, 33, 1, 20], np.int32)
SPK = np.array([2, -1, 0, 77, 5], np.int32)


def test_a_batch_row_equals_its_batch_1_call_and_the_pipeline_equals_the_serial_call(pkg, full_det):
    ids = pkg.synth_ids(5, 48)
    for mode in (0, 1):
        pcm, lengths, frames = full_det.process_batch(ids, id_lengths=LENS, mode=mode, noise_seed=9, speaker_ids=SPK)
        for b in range(5):
            one, l1, f1 = full_det.process_batch(ids[b:b + 1, :LENS[b]], mode=mode, noise_seed=9, noise_seed_offsets=[b], speaker_ids=SPK[b:b + 1])
            assert f1[0] == frames[b] and l1[0] == lengths[b]
            assert np.array_equal(one[0], pcm[b]), (mode, b)
    full_det.submit_batch(ids, id_lengths=LENS, mode=1, noise_seed=9, speaker_ids=SPK)
    full_det.submit_batch(ids, id_lengths=LENS, mode=1, noise_seed=9, speaker_ids=SPK)
    for _ in range(2):
        got, gl, gf = full_det.wait()
        np.testing.assert_array_equal(gf, frames)
        for x, y in zip(got, pcm):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("knob", [("VITS_NO_DP_DET_FUSE", "1"), ("VITS_DP_DET_LAT_MAX_BLOCKS", "0")], ids=["unfused", "wide-tile"])
def test_the_fused_kernel_equals_the_unfused_sequence_and_its_other_tile_on_the_whole_call(pkg, full_det, full_det_bytes, monkeypatch, knob):
    ids = pkg.synth_ids(5, 48)
    want, wl, wf = full_det.process_batch(ids, id_lengths=LENS, noise_seed=9, speaker_ids=SPK, collect_taps=True)
    want_logw = [full_det.tap("log_duration", b) for b in range(5)]
    monkeypatch.setenv(*knob)
    with pkg.Model(full_det_bytes) as m:  # (the knobs are read at load)
        got, gl, gf = m.process_batch(ids, id_lengths=LENS, noise_seed=9, speaker_ids=SPK, collect_taps=True)
        for b in range(5):
            assert np.array_equal(m.tap("log_duration", b), want_logw[b]), b
    np.testing.assert_array_equal(gf, wf)
    for x, y in zip(got, want):
        assert np.array_equal(x, y)


def test_no_speaker_equals_the_file_without_speaker_tensors_and_a_voice_equals_its_speaker(pkg, full_det):
    ids = pkg.synth_ids(3, 40)
    lens = np.array([40, 9, 27], np.int32)
    with pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL | pkg.SYNTH_DETERMINISTIC)) as base:
        want, wl, _ = base.process_batch(ids, id_lengths=lens, noise_seed=3)
    got, gl, _ = full_det.process_batch(ids, id_lengths=lens, noise_seed=3, speaker_ids=[-1, -1, -1])
    np.testing.assert_array_equal(gl, wl)
    for x, y in zip(got, want):
        assert np.array_equal(x, y)
    # speaker -1 beside a conditioned utterance reads row 0 of the table (zeros): still the same bits
    mixed, _, _ = full_det.process_batch(ids, id_lengths=lens, noise_seed=3, speaker_ids=[-1, 1, -1])
    assert np.array_equal(mixed[0], want[0]) and np.array_equal(mixed[2], want[2]) and not np.array_equal(mixed[1][:100], want[1][:100])
    (voice,) = full_det.add_voices(full_det.speaker_embedding(1))
    try:
        a, _, fa = full_det.process_batch(ids, id_lengths=lens, noise_seed=3, speaker_ids=[1, 1, 1])
        b, _, fb = full_det.process_batch(ids, id_lengths=lens, noise_seed=3, speaker_ids=[voice, voice, voice])
        np.testing.assert_array_equal(fa, fb)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    finally:
        full_det.clear_voices()


def test_prosody_options_behave_as_documented(pkg, full_det):
    ids = pkg.synth_ids(2, 24)
    lens = np.array([24, 11], np.int32)
    d0 = np.zeros((2, 24), np.int32)
    pcm, lengths, frames = full_det.process_batch(ids, id_lengths=lens, noise_seed=2, speaker_ids=[3, -1], durations_out=d0, collect_taps=True)
    logw = [full_det.tap("log_duration", b) for b in range(2)]
    for b in range(2):
        np.testing.assert_array_equal(d0[b, :lens[b]], np.ceil(np.exp(logw[b]) * np.float32(1.0)).astype(np.int32))
        assert d0[b].sum() == frames[b] and not d0[b, lens[b]:].any()
    # frames_only: the same frame counts, no audio
    _, l2, f2 = full_det.process_batch(ids, id_lengths=lens, noise_seed=2, speaker_ids=[3, -1], frames_only=True)
    np.testing.assert_array_equal(f2, frames)
    np.testing.assert_array_equal(l2, lengths)
    # speaking_rates: d = ceil(exp(logw) * (float)(1 / rate))
    d1 = np.zeros((2, 24), np.int32)
    full_det.process_batch(ids, id_lengths=lens, noise_seed=2, speaker_ids=[3, -1], speaking_rate=[0.5, 2.0], durations_out=d1, frames_only=True)
    for b, rate in enumerate((0.5, 2.0)):
        np.testing.assert_array_equal(d1[b, :lens[b]], np.ceil(np.exp(logw[b]) * np.float32(1.0 / rate)).astype(np.int32))
    # duration_override: >= 0 replaces, -1 keeps the prediction
    ovr = np.full((2, 24), -1, np.int32)
    ovr[0, 3], ovr[1, 0] = 9, 0
    d2 = np.zeros((2, 24), np.int32)
    _, _, f3 = full_det.process_batch(ids, id_lengths=lens, noise_seed=2, speaker_ids=[3, -1], duration_override=ovr, durations_out=d2, frames_only=True)
    want = d0.copy()
    want[0, 3], want[1, 0] = 9, 0
    np.testing.assert_array_equal(d2, want)
    np.testing.assert_array_equal(f3, want.sum(axis=1))
    # fixed_duration
    _, _, f4 = full_det.process_batch(ids, id_lengths=lens, fixed_duration=2, frames_only=True)
    np.testing.assert_array_equal(f4, 2 * lens)


def test_ggml_tables_mode_1_is_refused_and_mode_2_runs(pkg, full_det_bytes):
    ids = pkg.synth_ids(1, 12)
    with pkg.Model(full_det_bytes) as m:
        want, _, wf = m.process_batch(ids, noise_seed=1)
        m.set_ggml_tables(1)
        with pytest.raises(pkg.VitsError, match="deterministic duration predictor"):
            m.process_batch(ids, noise_seed=1)
        m.set_ggml_tables(2)
        got, _, gf = m.process_batch(ids, noise_seed=1)
        assert gf[0] > 0 and np.isfinite(got[0]).all()
        m.set_ggml_tables(0)
        again, _, _ = m.process_batch(ids, noise_seed=1)
        assert np.array_equal(again[0], want[0])


def test_every_arithmetic_mode_predicts_the_same_durations(pkg, full_det):
    ids = pkg.synth_ids(5, 48)
    frames = {}
    try:
        for scope in (pkg.SCOPE_FLOW_VOCODER, pkg.SCOPE_ALL_CONVS):
            full_det.set_arith_scope(scope)
            for arith in (pkg.ARITH_F32, pkg.ARITH_F16, pkg.ARITH_BF16, pkg.ARITH_F32_SPLIT):
                full_det.set_arith(arith)
                if scope == pkg.SCOPE_ALL_CONVS and arith in (pkg.ARITH_F16, pkg.ARITH_BF16):
                    continue  # (the text encoder then runs on 16-bit operands: the predictor's INPUT differs; its own convs stay fp32)
                _, _, frames[(scope, arith)] = full_det.process_batch(ids, id_lengths=LENS, noise_seed=9, speaker_ids=SPK, frames_only=True)
    finally:
        full_det.set_arith(pkg.ARITH_F32)
        full_det.set_arith_scope(pkg.SCOPE_FLOW_VOCODER)
    for k in frames:
        np.testing.assert_array_equal(frames[k], frames[(pkg.SCOPE_FLOW_VOCODER, pkg.ARITH_F32)], err_msg=str(k))


def test_alignment_and_conversion_run_and_the_alignment_reproduces_its_frames(pkg):
    """neither runs a duration predictor; the alignment's durations, fed back as duration_override, give frames[b]"""
    with pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_TINY | pkg.SYNTH_POSTERIOR | pkg.SYNTH_DETERMINISTIC)) as m:
        assert m.duration_predictor_kind == 1
        hop = m.hop
        rng = np.random.default_rng(4)
        lens = np.array([40 * hop + 3, 23 * hop], np.int64)
        pcm = (0.1 * rng.standard_normal((2, int(lens.max())))).astype(np.float32)
        tl = np.array([12, 7], np.int32)
        ids = pkg.synth_ids(2, 12)
        d, frames, scores = m.align_batch(pcm, ids, lens, tl)
        np.testing.assert_array_equal(frames, lens // hop)
        np.testing.assert_array_equal(d.sum(axis=1), frames)
        _, _, fr = m.process_batch(ids, tl, duration_override=d, noise_seed=3)
        np.testing.assert_array_equal(fr, frames)
        out, clen, cfr = m.convert_batch(pcm, lens, noise_seed=3)
        np.testing.assert_array_equal(cfr, frames)
        assert all(np.isfinite(o).all() for o in out)


def test_false_on_a_stochastic_file_is_refused_at_load(pkg):
    with open(os.path.join(GOLDEN, "tiny_speakers_hf_export.ggml"), "rb") as f:
        v, h, c, t = read_file(f.read())
    c = [(k, b"False" if k == b"use_stochastic_duration_prediction" else val) for k, val in c]
    with pytest.raises(pkg.VitsError, match="duration_predictor.conv_1.weight"):
        pkg.Model(write_file(v, h, c, t))
