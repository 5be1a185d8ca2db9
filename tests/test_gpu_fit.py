"""A stated duration at model level (vits_model_set_fit, vits_model_set_fit_total; include/vits.h "a stated duration"), through the C ABI: the durations of a fitted
group sum to its target; the call is, bit for bit, the same call with duration_override = its own durations_out; the durations are the numpy restatement
(tests/fit_ref.py) on the "fit_exp" tap; a clamped fit is a speaking_rates call; unfitted utterances and handles without a fit keep their bits; every entry
point gives the same bits; the refusals leave the handle usable and no fit behind.

The tiny golden models (stochastic, deterministic, with speakers) and the synthetic tiny model, four ragged utterances of at most 24 ids. Nothing here has a
tolerance."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
import fit_ref as FR

pytestmark = pytest.mark.gpu

LENS = np.array([5, 12, 24, 17], np.int32)
GOLDEN_MODELS = ("tiny_hf_export.ggml", "tiny_detdp_hf_export.ggml", "tiny_speakers_hf_export.ggml")


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)


def same_result(got, want):
    return np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and len(got[0]) == len(want[0]) and all(same(a, b) for a, b in zip(got[0], want[0]))


@pytest.fixture(scope="module")
def models(pkg, tiny_bytes):
    """name -> (model, ids [4, 24]); opened once"""
    out = {}
    blobs = {"synth": tiny_bytes}
    for name in GOLDEN_MODELS:
        with open(os.path.join(GOLDEN, name), "rb") as f:
            blobs[name] = f.read()
    for name, blob in blobs.items():
        m = pkg.Model(blob)
        out[name] = (m, pkg.synth_ids(4, 24, vocab=m.vocab_size))
    yield out
    for m, _ in out.values():
        m.close()


@pytest.fixture()
def tiny(pkg, models):
    m, ids = models["synth"]
    m.set_fit(None)
    m.set_arith(pkg.ARITH_F32)
    yield m, ids
    m.set_fit(None)
    m.set_arith(pkg.ARITH_F32)


def call(m, ids, **kw):
    return m.process_batch(ids, id_lengths=LENS, noise_seed=7, **kw)


def natural(m, ids, **kw):
    dur = np.zeros((4, 24), np.int32)
    frames = call(m, ids, frames_only=True, durations_out=dur, **kw)[2]
    assert np.array_equal(frames, np.maximum(1, dur.sum(axis=1)))
    return frames, dur


def group_sums(dur, groups, B=4):
    n = np.zeros(B, np.int64)
    for b in range(B):
        n[groups[b]] += dur[b].sum()
    return n


def test_a_fitted_group_lasts_its_target(pkg, tiny):
    m, ids = tiny
    frames0, _ = natural(m, ids)
    for groups in (None, [0, 0, 0, 0], [2, 0, 2, 0]):
        g = np.arange(4) if groups is None else np.array(groups)
        base = group_sums(frames0[:, None], g)
        for factor in (0.6, 0.93, 1.0, 1.07, 1.9):
            targets = np.where(base > 0, np.maximum(1, (base * factor).astype(np.int64) + (factor == 1.07)), 0)
            dur = np.zeros((4, 24), np.int32)
            fit = dict(targets=targets, groups=groups)
            pcm, lengths, frames = call(m, ids, durations_out=dur, fit=fit)
            rows = m.last_fit()
            assert rows.shape == (4, 6) and np.array_equal(rows[:, 0], g)
            assert np.array_equal(group_sums(dur, g), targets) and np.array_equal(frames, dur.sum(axis=1))
            for b in range(4):
                assert rows[b, 1] == rows[b, 2] == targets[g[b]] and rows[b, 5] == 0 and (dur[b, LENS[b]:] == 0).all()
                assert lengths[b] == pcm[b].size
            # frames_only: the same durations, frames and report, no audio
            dur2 = np.zeros((4, 24), np.int32)
            none, lengths2, frames2 = call(m, ids, durations_out=dur2, fit=fit, frames_only=True)
            assert none is None and np.array_equal(dur2, dur) and np.array_equal(frames2, frames) and np.array_equal(lengths2, lengths)
            assert np.array_equal(m.last_fit(), rows)
    # a call without a fit reports none
    call(m, ids, frames_only=True)
    assert m.last_fit() is None


@pytest.mark.parametrize("name,arith,speakers", [("tiny_hf_export.ggml", "ARITH_F32", None), ("tiny_hf_export.ggml", "ARITH_F16", None),
                                                 ("tiny_detdp_hf_export.ggml", "ARITH_F32", None), ("tiny_detdp_hf_export.ggml", "ARITH_F16", None),
                                                 ("tiny_speakers_hf_export.ggml", "ARITH_F32", [1, 0, -1, 1])])
def test_the_call_is_the_call_with_its_own_durations_stated(pkg, models, name, arith, speakers):
    m, ids = models[name]
    m.set_arith(getattr(pkg, arith))
    try:
        kw = dict(speaker_ids=speakers) if speakers else {}
        frames0, _ = natural(m, ids, **kw)
        # groups {0, 2} and {1}; utterance 3 is not fitted; one token of utterance 2 is the caller's
        groups = [0, 1, 0, 3]
        targets = [int((frames0[0] + frames0[2]) * 1.31), max(1, int(frames0[1] * 0.77)), 0, 0]
        ovr = np.full((4, 24), -1, np.int32)
        ovr[2, 3] = 9
        ovr[3, 1] = 0
        dur = np.zeros((4, 24), np.int32)
        got = call(m, ids, durations_out=dur, duration_override=ovr, fit=dict(targets=targets, groups=groups), collect_taps=True, **kw)
        rows = m.last_fit()
        assert dur[2, 3] == 9 and dur[3, 1] == 0 and dur[0].sum() + dur[2].sum() == targets[0] and dur[1].sum() == targets[1]
        assert rows[:, 5].tolist() == [0, 0, 0, -1] and rows[3, 1] == 0
        # the restatement on the tap: every integer, and the scale's bits
        e = np.zeros((4, 24), np.float32)
        for b in range(4):
            e[b, :LENS[b]] = m.tap("fit_exp", b)
            assert np.abs(e[b, :LENS[b]] / np.exp(m.tap("log_duration", b).astype(np.float64)) - 1).max() < 4e-7  # (the device library's expf)
        w_dur, w_rows = FR.fit(e, targets, LENS, ovr, groups)
        for b in range(3):
            assert np.array_equal(dur[b, :LENS[b]], w_dur[b, :LENS[b]]), b
            assert np.array_equal(rows[b, 1:].view(np.uint64), w_rows[groups[b]].view(np.uint64)), b
        # ... and the PCM is that of the call that states those durations
        want = call(m, ids, duration_override=dur, **kw)
        assert same_result(got, want)
        assert m.last_fit() is None
        # the unfitted utterance is the one of the call without a fit
        plain = call(m, ids, duration_override=ovr, **kw)
        assert same(got[0][3], plain[0][3]) and got[2][3] == plain[2][3]
    finally:
        m.set_arith(pkg.ARITH_F32)


def test_a_clamped_fit_is_the_speaking_rate(pkg, tiny):
    m, ids = tiny
    got = call(m, ids, fit=dict(targets=[1, 1, 1, 1], min_rate=0.5, max_rate=1.5))
    rows = m.last_fit()
    assert (rows[:, 5] == 1).all() and (rows[:, 2] > 1).all() and (rows[:, 3].astype(np.float32) == np.float32(1.0 / 1.5)).all()
    assert same_result(got, call(m, ids, speaking_rate=1.5))
    got = call(m, ids, fit=dict(frames=1 << 22, min_rate=0.5, max_rate=1.5))
    assert (m.last_fit()[:, 5] == 2).all() and same_result(got, call(m, ids, speaking_rate=0.5))
    # (the model-level rate and speaking_rates are validated and not used by a fitted utterance)
    frames0, _ = natural(m, ids)
    a = call(m, ids, fit=dict(targets=frames0 + 3))
    b = call(m, ids, fit=dict(targets=frames0 + 3), speaking_rate=[0.5, 2.0, 1.0, 3.0])
    assert same_result(a, b)
    with pytest.raises(pkg.VitsError, match=r"speaking_rates\[1\]"):
        call(m, ids, fit=dict(targets=frames0 + 3), speaking_rate=[0.5, 20.0, 1.0, 3.0])


def test_groups_of_one_are_separate_calls_and_every_entry_point_agrees(pkg, tiny):
    m, ids = tiny
    frames0, _ = natural(m, ids)
    targets = (frames0 * np.array([1.2, 0.8, 1.05, 1.5])).astype(np.int64)
    dur = np.zeros((4, 24), np.int32)
    want = call(m, ids, fit=dict(targets=targets), durations_out=dur)
    rows = m.last_fit()
    assert np.array_equal(want[2], targets)
    for b in range(4):
        one = m.process_batch(ids[b:b + 1], id_lengths=LENS[b:b + 1], noise_seed=7, noise_seed_offsets=[b], fit=int(targets[b]))
        assert same(one[0][0], want[0][b]) and one[2][0] == targets[b]
        assert np.array_equal(m.last_fit()[0, 1:], rows[b, 1:])
    # the pipeline: two batches in flight, each wait reports its own batch
    d2 = np.zeros((4, 24), np.int32)
    m.submit_batch(ids, id_lengths=LENS, noise_seed=7, fit=dict(targets=targets), durations_out=d2)
    m.submit_batch(ids[:2], id_lengths=LENS[:2], noise_seed=7)
    assert same_result(m.wait(), want) and np.array_equal(m.last_fit(), rows) and np.array_equal(d2, dur)
    m.wait()
    assert m.last_fit() is None
    # vocoder windows, with and without a sink: the timings arrive first, the bits stay
    assert same_result(call(m, ids, fit=dict(targets=targets), vocoder_chunk_frames=7), want)
    chunks = []
    got = call(m, ids, fit=dict(targets=targets), vocoder_chunk_frames=7, on_chunk=lambda utt, off, pcm: chunks.append((utt, off, pcm.size)) and False)
    assert same_result(got, want) and chunks
    # a batch large enough to be split inside the call stays whole when it fits: one group over all of it
    big = np.tile(ids, (4, 1))
    big_lens = np.tile(LENS, 4)
    total = int(np.tile(frames0, 4).sum() * 1.1)
    d16 = np.zeros((16, 24), np.int32)
    m.process_batch(big, id_lengths=big_lens, noise_seed=7, fit=total, durations_out=d16)
    assert d16.sum() == total and (m.last_fit()[:, 5] == 0).all() and m.last_fit().shape == (16, 6)


def test_a_joined_call_and_a_spoken_text_take_a_total(pkg, tiny):
    m, ids = tiny
    frames0, _ = natural(m, ids)
    total = int(frames0.sum() * 1.25)
    dur = np.zeros((4, 24), np.int32)
    pcm, lengths, frames = m.process_joined(ids, id_lengths=LENS, track=[0, 0, 1, 1], gap_ms=[0, 30, 0, 10], noise_seed=7, fit=total, durations_out=dur)
    joins, rows = m.last_joins(), m.last_fit()
    assert frames.sum() == dur.sum() == total and (rows[:, 5] == 0).all() and (rows[:, 2] == total).all() and (rows[:, 0] == 0).all()
    assert np.array_equal(frames, [dur[:2].sum(), dur[2:].sum()])
    # last_joins is consistent: every utterance has the samples of the plain call that states those durations, and the joined call is that call joined
    assert np.array_equal(joins[:, 3], call(m, ids, duration_override=dur)[1])
    want = m.process_joined(ids, id_lengths=LENS, track=[0, 0, 1, 1], gap_ms=[0, 30, 0, 10], noise_seed=7, duration_override=dur)
    assert same_result((pcm, lengths, frames), want) and np.array_equal(m.last_joins(), joins)
    # per group in a joined call
    per = [int(frames0[:2].sum() * 0.9), int(frames0[2:].sum() * 1.2)]
    _, _, frames = m.process_joined(ids, id_lengths=LENS, track=[0, 0, 1, 1], noise_seed=7, fit=dict(targets=per + [0, 0], groups=[0, 0, 1, 1]))
    assert np.array_equal(frames, per) and np.array_equal(m.last_fit()[[0, 2], 2], per)
    # a whole text in a stated time
    text = "hello there. what now? ok"
    _, _, f0 = m.speak(text, sentence_gap_ms=50, noise_seed=3, frames_only=True)
    want = int(f0.sum() * 0.8)
    pcm, lengths, frames = m.speak(text, sentence_gap_ms=50, noise_seed=3, fit=want)
    assert frames.sum() == want and (m.last_fit()[:, 5] == 0).all() and (m.last_fit()[:, 2] == want).all()
    # the frames-to-samples rule: samples = frames * hop + sadd, both read off a plain call
    _, n1, f1 = call(m, ids)
    sadd = int(n1[0] - f1[0] * m.hop)
    assert np.array_equal(n1, f1 * m.hop + sadd)
    for L in (1, 2, want, 12345):
        assert m.fit_frames((L * m.hop + sadd + 0.5) / m.sampling_rate) == L and m.fit_frames((L * m.hop + sadd - 0.5) / m.sampling_rate) == max(L - 1, 1)
    assert m.fit_frames(0.0) == 1
    with pytest.raises(pkg.VitsError, match="vits_model_speak: the targets of vits_model_set_fit are one per group"):
        m.speak(text, fit=dict(targets=[want]))
    m.speak(text, noise_seed=3)
    assert m.last_fit() is None


def test_refusals_leave_the_handle_usable_and_no_fit_behind(pkg, tiny):
    m, ids = tiny
    before = call(m, ids)
    frames0 = before[2]
    ok = dict(targets=frames0 + 1)
    for kw, msg in (
        (dict(fit=ok, fixed_duration=3), "fixed_duration > 0 leaves the duration predictor nothing to scale"),
        (dict(fit=ok, async_=True, skip_host_copy=True), "async returns before the device has finished"),
        (dict(fit=ok, pitch_ratio=[1.0, 1.2, 1.0, 1.0]), r"utterance 1 of the fitted group 1 has the pitch ratio"),
        (dict(fit=dict(targets=[5, 5, 5])), r"n = 3 was given, and this call has 4 utterances"),
        (dict(fit=dict(targets=[5, 5, 5, (1 << 22) + 1])), r"target_frames\[3\] = 4194305 \(group 3\)"),
        (dict(fit=dict(targets=[5, 5, 5, -2])), r"target_frames\[3\] = -2"),
        (dict(fit=dict(targets=[5, 5, 5, 5], groups=[0, 1, 2, 4])), r"groups\[3\] = 4"),
        (dict(fit=dict(targets=[5, 5, 5, 5], min_rate=0.01)), r"0.1 <= min_rate <= max_rate <= 10"),
        (dict(fit=dict(frames=0)), r"vits_model_set_fit_total: total_frames = 0: a target is 1 to 2\^22 frames"),
    ):
        with pytest.raises(pkg.VitsError, match=msg):
            call(m, ids, **kw)
        assert same_result(call(m, ids), before), kw  # no fit was left behind, and the handle gives what it gave
        assert m.last_fit() is None
    # a pitch on an utterance that is NOT fitted is fine
    call(m, ids, fit=dict(targets=[int(frames0[0]) + 2, 0, 0, 0]), pitch_ratio=[1.0, 1.2, 1.0, 1.0])
    assert m.last_fit()[:, 5].tolist() == [0, -1, -1, -1]
    # the exact-order stage one
    m.set_ggml_tables(1)
    try:
        with pytest.raises(pkg.VitsError, match=r"vits_model_set_ggml_tables\(model, 1\)"):
            call(m, ids, fit=ok)
    finally:
        m.set_ggml_tables(0)
    # conversion and alignment predict no durations
    pcm = np.zeros((1, 4000), np.float32)
    with pytest.raises(pkg.VitsError, match="voice conversion does not take the fit"):
        m.convert_batch(pcm, fit=100)
    with pytest.raises(pkg.VitsError, match="alignment does not take the fit"):
        m.align_batch(pcm, ids[:1, :5], fit=100)
    # a fit given through the C entry point is taken by the next call, whatever becomes of it, and by that call alone
    m.set_fit(frames0 + 1)
    with pytest.raises(pkg.VitsError, match="fixed_duration"):
        call(m, ids, fixed_duration=2)
    assert same_result(call(m, ids), before)
    m.set_fit(frames0 + 1)
    m.set_fit(None)
    assert same_result(call(m, ids), before)
    m.set_fit_total(int(frames0.sum()) + 4)
    assert call(m, ids)[2].sum() == frames0.sum() + 4
    assert same_result(call(m, ids), before)


def test_with_nothing_set_every_bit_is_what_it_was(pkg, tiny, tiny_bytes):
    _, ids = tiny
    with pkg.Model(tiny_bytes) as a, pkg.Model(tiny_bytes) as b:
        want = call(b, ids)
        call(a, ids, fit=dict(targets=want[2] * 2))  # a handle that has fitted ...
        assert a.last_fit() is not None
        got = call(a, ids)  # ... and one that never heard of it
        assert same_result(got, want) and a.last_fit() is None and b.last_fit() is None
        assert a.weight_bytes == b.weight_bytes
        # every target 0: nothing is fitted, nothing is reported
        assert same_result(call(a, ids, fit=dict(targets=[0, 0, 0, 0])), want) and a.last_fit() is None
