"""Speaker conditioning on the GPU (multi-speaker models): against transformers.VitsModel(speaker_id=...) taps
(tests/golden/make_golden_speakers.py), per-utterance speakers in one batch, the pipeline / split / windowed / frames-only paths,
kernel choices, the default speaker and every refusal."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def export_bytes():
    with open(os.path.join(GOLDEN, "tiny_speakers_hf_export.ggml"), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def full_spk_bytes(pkg):
    return pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL | pkg.SYNTH_SPEAKERS)


@pytest.fixture(scope="module")
def full_spk(pkg, full_spk_bytes):
    m = pkg.Model(full_spk_bytes)
    yield m
    m.close()


def key(s):
    return "sm1" if s < 0 else "s%d" % s


@pytest.mark.parametrize("fixture,mode", [("tiny_speakers_hf_export_taps.npz", 1), ("tiny_speakers_hf_export_refmode_taps.npz", 0),
                                          ("full_synth_speakers_taps.npz", 1), ("full_synth_speakers_refmode_taps.npz", 0)])
def test_speakers_match_transformers_taps(pkg, export_bytes, full_spk_bytes, fixture, mode):
    g = golden(fixture)
    dec = int(g["decimate"][0])
    with pkg.Model(export_bytes if fixture.startswith("tiny") else full_spk_bytes) as m:
        assert m.num_speakers == (3 if fixture.startswith("tiny") else 109)
        for s in g["speakers"].tolist():
            k = key(s)
            pcm, lengths, _ = m.process_batch(g["ids"], mode=mode, noise_kind=pkg.NOISE_EXPLICIT, noise_dur=g["noise_dur"][None],
                                              noise_prior=g[k + "_noise_prior"][None], collect_taps=True, speaker_ids=[s])
            np.testing.assert_array_equal(m.tap("durations"), g[k + "_durations"].ravel(), err_msg=k)
            assert rel_err(m.tap("log_duration"), g[k + "_log_duration"]) < 2e-4, k
            assert rel_err(m.tap("z_flow"), g[k + "_z_flow"]) < 2e-4, k
            assert lengths[0] == int(g[k + "_waveform_len"][0]), k
            assert rel_err(pcm[0][::dec], g[k + "_waveform"]) < 2e-4, k
        frames = {s: int(g[key(s) + "_durations"].sum()) for s in g["speakers"].tolist()}
        assert len(set(frames.values())) > 1  # the fixture's speakers really move the durations


def test_speakers_f16_match_the_torch_operand_rounding_fixture(pkg):
    """VITS_ARITH_F16 (default scope), reference mode, with conditioning, on the tiny synthetic speaker model (the architecture and weights of
    test_gpu_arith16.py's tiny rounding fixture + the speaker tensors): that test's tolerance (f16: 5e-3 max, a quarter of it RMS)."""
    g = golden("tiny_synth_speakers_arith_f16_taps.npz")
    tol = 5e-3
    with pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_TINY | pkg.SYNTH_SPEAKERS)) as m:
        m.set_arith(pkg.ARITH_F16)
        for s in g["speakers"].tolist():
            k = key(s)
            pcm, lengths, _ = m.process_batch(g["ids"], mode=pkg.MODE_REFERENCE, noise_kind=pkg.NOISE_EXPLICIT, noise_dur=g["noise_dur"][None],
                                              noise_prior=g[k + "_noise_prior"][None], collect_taps=True, speaker_ids=[s])
            np.testing.assert_array_equal(m.tap("durations"), g[k + "_durations"].ravel(), err_msg=k)
            assert lengths[0] == int(g[k + "_waveform_len"][0])
            for a, b in ((m.tap("z_flow"), g[k + "_z_flow"]), (pcm[0], g[k + "_waveform"])):
                a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
                rms = np.sqrt((b ** 2).mean())
                assert np.abs(a - b).max() / rms < tol and np.sqrt(((a - b) ** 2).mean()) / rms < tol / 4, k


def test_no_speaker_on_a_speaker_model_equals_the_single_speaker_model(pkg, full_spk, full_bytes):
    """VITS_SYNTH_SPEAKERS only appends tensors: speaker -1 must reproduce the single-speaker model bit for bit (row 0 = the plain biases)."""
    ids = pkg.synth_ids(3, 40)
    lens = np.array([40, 9, 27], np.int32)
    with pkg.Model(full_bytes) as base:
        for arith in (pkg.ARITH_F32, pkg.ARITH_F16):
            base.set_arith(arith)
            full_spk.set_arith(arith)
            want, wl, _ = base.process_batch(ids, id_lengths=lens, noise_seed=3)
            got, gl, _ = full_spk.process_batch(ids, id_lengths=lens, noise_seed=3, speaker_ids=[-1, -1, -1])
            np.testing.assert_array_equal(gl, wl)
            for x, y in zip(got, want):
                assert np.array_equal(x, y)
    full_spk.set_arith(pkg.ARITH_F32)


MIX = np.array([2, -1, 0, 1, 2, 0], np.int32)
MIX_LENS = np.array([48, 7, 33, 48, 1, 20], np.int32)


def test_mixed_batch_rows_equal_their_batch_one_calls(pkg, full_spk):
    ids = pkg.synth_ids(6, 48)
    full_spk.set_arith(pkg.ARITH_F32)
    for mode in (0, 1):
        pcm, lengths, frames = full_spk.process_batch(ids, id_lengths=MIX_LENS, mode=mode, noise_seed=9, speaker_ids=MIX)
        for b in range(6):
            one, l1, f1 = full_spk.process_batch(ids[b:b + 1, :MIX_LENS[b]], mode=mode, noise_seed=9, noise_seed_offsets=[b], speaker_ids=MIX[b:b + 1])
            assert f1[0] == frames[b] and l1[0] == lengths[b]
            assert np.array_equal(one[0], pcm[b]), (mode, b)


def test_durations_do_not_depend_on_the_arithmetic_mode(pkg, full_spk):
    ids = pkg.synth_ids(6, 48)
    frames = {}
    for arith in (pkg.ARITH_F32, pkg.ARITH_F16, pkg.ARITH_BF16, pkg.ARITH_F32_SPLIT):
        full_spk.set_arith(arith)
        _, _, frames[arith] = full_spk.process_batch(ids, id_lengths=MIX_LENS, noise_seed=9, speaker_ids=MIX)
    full_spk.set_arith(pkg.ARITH_F32)
    for a in frames:
        np.testing.assert_array_equal(frames[a], frames[pkg.ARITH_F32])


def test_speakers_change_durations_and_audio(pkg, full_spk):
    ids = np.repeat(pkg.synth_ids(1, 40), 4, axis=0)
    pcm, _, frames = full_spk.process_batch(ids, noise_seed=4, noise_seed_offsets=[0, 0, 0, 0], speaker_ids=[-1, 0, 1, 108])
    assert len(set(frames.tolist())) > 1
    for a in range(4):
        for b in range(a + 1, 4):
            assert pcm[a].size != pcm[b].size or not np.array_equal(pcm[a], pcm[b]), (a, b)


@pytest.mark.parametrize("arith", ["f32", "f16"])
def test_pipelined_windowed_and_frames_only_equal_process_batch(pkg, full_spk, arith):
    full_spk.set_arith(pkg.ARITH_F32 if arith == "f32" else pkg.ARITH_F16)
    ids = pkg.synth_ids(6, 120, ids_seed=5)
    lens = np.array([120, 17, 90, 64, 3, 111], np.int32)
    spk = np.array([5, -1, 0, 108, 5, 60], np.int32)
    want, wl, wf = full_spk.process_batch(ids, id_lengths=lens, noise_seed=2, speaker_ids=spk)
    # pipelined: the speakers are copied at submit (the caller's array is overwritten before the wait)
    arr = spk.copy()
    full_spk.submit_batch(ids, id_lengths=lens, noise_seed=2, speaker_ids=arr)
    arr[:] = 7
    full_spk.submit_batch(ids[::-1].copy(), id_lengths=lens[::-1].copy(), noise_seed=2, speaker_ids=spk[::-1].copy(), noise_seed_offsets=np.arange(6)[::-1].copy())
    got, gl, gf = full_spk.wait()
    got2, _, _ = full_spk.wait()
    np.testing.assert_array_equal(gf, wf)
    for b in range(6):
        assert np.array_equal(got[b], want[b]) and np.array_equal(got2[5 - b], want[b]), b
    # windowed vocoder
    win, _, _ = full_spk.process_batch(ids, id_lengths=lens, noise_seed=2, speaker_ids=spk, vocoder_chunk_frames=40)
    for b in range(6):
        assert np.array_equal(win[b], want[b]), b
    # frames only
    _, fl, ff = full_spk.process_batch(ids, id_lengths=lens, noise_seed=2, speaker_ids=spk, frames_only=True)
    np.testing.assert_array_equal(ff, wf)
    np.testing.assert_array_equal(fl, wl)
    full_spk.set_arith(pkg.ARITH_F32)


def test_in_call_split_equals_the_unsplit_call(pkg, full_spk_bytes, monkeypatch):
    ids = pkg.synth_ids(8, 64, ids_seed=3)
    lens = np.array([64, 5, 40, 64, 12, 1, 33, 50], np.int32)
    spk = np.array([3, -1, 3, 100, 0, -1, 7, 50], np.int32)
    monkeypatch.setenv("VITS_SPLIT_MIN_BATCH", "0")
    with pkg.Model(full_spk_bytes) as m:
        want, wl, wf = m.process_batch(ids, id_lengths=lens, noise_seed=8, speaker_ids=spk)
    monkeypatch.setenv("VITS_SPLIT_MIN_BATCH", "2")
    with pkg.Model(full_spk_bytes) as m:
        got, gl, gf = m.process_batch(ids, id_lengths=lens, noise_seed=8, speaker_ids=spk)
    np.testing.assert_array_equal(gf, wf)
    for b in range(8):
        assert np.array_equal(got[b], want[b]), b


def test_default_speaker_drives_the_reference_entry_points(pkg, export_bytes):
    with pkg.Model(export_bytes) as m:
        assert m.speaker == -1
        ids = pkg.synth_ids(1, 20)[0]
        pkg.lib().vits_reference_noise_seed(1)
        a = m.process_ids(ids)
        m.set_speaker(2)
        assert m.speaker == 2
        pkg.lib().vits_reference_noise_seed(1)
        b = m.process_ids(ids)
        c, _, _ = m.process_batch(ids[None], noise_seed=3)  # speaker_ids=None: the default too
        d, _, _ = m.process_batch(ids[None], noise_seed=3, speaker_ids=[2])
        assert np.array_equal(c[0], d[0])
        m.set_speaker(-1)
        e, _, _ = m.process_batch(ids[None], noise_seed=3)
        assert not np.array_equal(e[0], d[0]) or e[0].size != d[0].size
        assert a.size != b.size or not np.array_equal(a, b)


def test_refusals_name_the_utterance(pkg, export_bytes, full_bytes):
    ids = pkg.synth_ids(3, 10)
    with pkg.Model(export_bytes) as m:
        for bad in ([0, 3, 1], [0, -2, 1]):
            with pytest.raises(pkg.VitsError, match=r"speaker_ids\[1\]"):
                m.process_batch(ids, speaker_ids=bad)
            with pytest.raises(pkg.VitsError, match=r"speaker_ids\[1\]"):
                m.submit_batch(ids, speaker_ids=bad)
        for bad in (3, -2):
            with pytest.raises(pkg.VitsError, match="outside"):
                m.set_speaker(bad)
        m.set_ggml_tables(1)
        with pytest.raises(pkg.VitsError, match=r"speaker_ids\[2\].*set_ggml_tables"):
            m.process_batch(ids, speaker_ids=[-1, -1, 1])
        m.process_batch(ids, speaker_ids=[-1, -1, -1])
        m.set_ggml_tables(2)
        m.process_batch(ids, speaker_ids=[-1, 0, 1])
    with pkg.Model(full_bytes) as m:
        assert m.num_speakers == 1
        with pytest.raises(pkg.VitsError, match=r"speaker_ids\[0\].*single speaker"):
            m.process_batch(ids, speaker_ids=[0, -1, -1])
        with pytest.raises(pkg.VitsError, match="single speaker"):
            m.set_speaker(0)
        m.process_batch(ids, speaker_ids=[-1, -1, -1])


def test_kernel_choices_do_not_change_a_single_bit_with_speakers():
    """The knob sets of test_tuning_knobs_do_not_change_a_single_bit / test_16bit_kernel_choices_do_not_change_a_single_bit that switch between
    variants of the speaker-conditioned layers (generic / latency convs, fused WaveNet layers, fused coupling layers, the DDS head), on the
    FULL speaker model with mixed speakers (tools/speaker_knob_identity.py): no variant that lacks the per-utterance bias may be chosen."""
    script = os.path.join(ROOT, "tools", "speaker_knob_identity.py")

    def run(arith, extra):
        env = dict(os.environ)
        env.update(extra)
        env["VITS_KNOB_ARITH"] = arith
        out = subprocess.run([sys.executable, script], env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        return out.stdout.strip().splitlines()[-1]

    sets = {
        "f32": [{"VITS_NO_ONESHOT": "1"}, {"VITS_NO_NARROW": "1"}, {"VITS_TILE128": "0", "VITS_NARROW_TILES": "0"}, {"VITS_MIN_BLOCKS": "100000"},
                {"VITS_NO_LAT16": "1"}, {"VITS_LAT16_MAX_WAVES": "0"}, {"VITS_LAT16_MAX_WAVES": "100000"}, {"VITS_NO_DDS_FUSE": "1"},
                {"VITS_NO_WN_FUSE": "1"}, {"VITS_DB_MIN": "2", "VITS_NBUF": "3"}, {"VITS_NARROW_K1": "0", "VITS_MIN_BLOCKS": "512"},
                {"VITS_NO_ONESHOT": "1", "VITS_NO_NARROW": "1", "VITS_NO_DDS_FUSE": "1", "VITS_NO_FUSE32": "1", "VITS_NO_WN_FUSE": "1"}],
        "f16": [{"VITS_NO_FLOW_FUSE": "1"}, {"VITS_FLOW_NCW": "1"}, {"VITS_NO_FLOW_FUSE": "1", "VITS_NO_WN_FUSE": "1"}, {"VITS_NO_FLOW_FUSE": "1", "VITS_WN16_NCW": "2"},
                {"VITS_NO_LAT16": "1"}, {"VITS_FLOW_NARROW_MAX": "0"}, {"VITS_FLOW_NARROW_MAX": "100000"}, {"VITS_NO_DDS_LAT": "1"}, {"VITS_DDS_LAT_MAX_BLOCKS": "2"},
                {"VITS_NO_LAT16H": "1"}, {"VITS_NO_LAT16H_PRE": "1"}, {"VITS_FLOW_CHAINS": "1"}],
    }
    for arith, knob_sets in sets.items():
        base = run(arith, {})
        for extra in knob_sets:
            assert run(arith, extra) == base, (arith, extra)
