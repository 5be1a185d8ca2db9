"""Custom voices on the GPU (vits_model_add_voices, voices.hip): speaker embeddings registered at run time. Exact identities — a voice that is a file
speaker is that speaker, a voice equals a model file that holds its vector, registration order and table growth change nothing, a mixed batch equals its
rows — through text-to-speech, conversion and alignment; the same kernels as file speakers; memory accounting; every refusal; and transformers taps
for blended and random vectors (tests/golden/make_golden_voices.py)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden, rel_err
from modelfile_py import parse_model_file

pytestmark = pytest.mark.gpu

ARITHS = ("ARITH_F32", "ARITH_F16", "ARITH_BF16", "ARITH_F32_SPLIT")


@pytest.fixture(scope="module")
def export_bytes():
    with open(os.path.join(GOLDEN, "tiny_speakers_hf_export.ggml"), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def full_spk_bytes(pkg):
    return pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL | pkg.SYNTH_SPEAKERS)


@pytest.fixture(scope="module")
def full_vc_bytes(pkg):
    return pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL | pkg.SYNTH_SPEAKERS | pkg.SYNTH_POSTERIOR)


def tts(m, ids, spk, lens=None, **kw):
    """(pcm list, lengths, frames, durations_out) of one process_batch call with counter noise and a fixed seed"""
    ids = np.atleast_2d(np.asarray(ids, np.int32))
    d = np.zeros(ids.shape, np.int32)
    kw.setdefault("noise_seed", 7)
    pcm, lengths, frames = m.process_batch(ids, id_lengths=lens, speaker_ids=spk, durations_out=d, **kw)
    return pcm, lengths, frames, d


def same(got, want, what=""):
    """two tts() / convert_batch() results are bit-identical: PCM, lengths, frames and durations"""
    for k in range(1, len(want)):
        np.testing.assert_array_equal(got[k], want[k], err_msg=str(what))
    assert (got[0] is None) == (want[0] is None), what
    for b, (x, y) in enumerate(zip(got[0] or [], want[0] or [])):
        np.testing.assert_array_equal(x, y, err_msg="%s utterance %d" % (what, b))


def signals(n_list, seed=5):
    rng = np.random.default_rng(seed)
    out = np.zeros((len(n_list), max(n_list)), np.float32)
    for b, n in enumerate(n_list):
        t = np.arange(n) / 16000.0
        y = np.sin(2 * np.pi * rng.uniform(100, 250) * t) + 0.3 * np.sin(2 * np.pi * rng.uniform(400, 900) * t) + 0.05 * rng.standard_normal(n)
        out[b, :n] = 0.8 * y / np.abs(y).max()
    return out, np.array(n_list, np.int64)


def with_row(data, row, vec):
    """a copy of the model file in which embed_speaker row `row` holds vec (the tensor is fp32: the row's bytes are overwritten in place)"""
    emb, dt = parse_model_file(data)["tensors"]["embed_speaker.weight"]
    assert dt == 0 and emb.dtype == np.float32 and emb.shape[1] == vec.size
    old = emb[row].tobytes()
    assert data.count(old) == 1
    at = data.find(old)
    out = data[:at] + np.asarray(vec, np.float32).tobytes() + data[at + len(old):]
    assert len(out) == len(data)
    return out


# ---- 3. a voice that is a file speaker is that speaker -------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["tiny", "full"])
def test_a_voice_that_is_a_file_speaker_is_that_speaker(pkg, export_bytes, full_spk_bytes, which):
    data, speakers = (export_bytes, [0, 1, 2]) if which == "tiny" else (full_spk_bytes, [0, 57, 108])
    ids = pkg.synth_ids(1, 24, ids_seed=3)
    with pkg.Model(data) as m:
        N, E = m.num_speakers, m.speaker_embedding_size
        assert (N, E) == ((3, 8) if which == "tiny" else (109, 256)) and m.num_voices == 0
        voices = m.add_voices(np.stack([m.speaker_embedding(s) for s in speakers]))
        assert voices == [N + k for k in range(len(speakers))] and m.num_voices == len(speakers) and m.num_speakers == N
        for arith in ARITHS:
            m.set_arith(getattr(pkg, arith))
            for mode in (0, 1):
                for s, v in zip(speakers, voices):
                    same(tts(m, ids, [v], mode=mode), tts(m, ids, [s], mode=mode), (arith, mode, s))


# ---- 4. a voice equals a file that holds it ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["tiny", "full"])
@pytest.mark.parametrize("vector", ["blend", "random"])
def test_a_voice_equals_a_model_file_that_holds_it(pkg, export_bytes, full_vc_bytes, which, vector):
    data = export_bytes if which == "tiny" else full_vc_bytes
    hop = 8 if which == "tiny" else 256
    T = 10
    ids = pkg.synth_ids(2, T, ids_seed=4)
    rec, rec_lens = signals([hop * 37, hop * 25], seed=6)
    with pkg.Model(data) as m:
        E = m.speaker_embedding_size
        if vector == "blend":
            vec = (np.float32(0.5) * m.speaker_embedding(0) + np.float32(0.5) * m.speaker_embedding(1)).astype(np.float32)
        else:
            vec = np.random.default_rng(21).standard_normal(E).astype(np.float32)
        with pkg.Model(with_row(data, 2, vec)) as f:
            np.testing.assert_array_equal(f.speaker_embedding(2), vec)
            v = m.add_voices(vec)[0]
            np.testing.assert_array_equal(m.speaker_embedding(v), vec)
            assert m.hop == hop
            for arith in ("ARITH_F32", "ARITH_F16"):
                m.set_arith(getattr(pkg, arith))
                f.set_arith(getattr(pkg, arith))
                for mode in (0, 1):
                    same(tts(m, ids, [v, 1], mode=mode), tts(f, ids, [2, 1], mode=mode), ("tts", arith, mode))
                    for (sv, tv), (sf, tf) in ((([v, v], [1, 0]), ([2, 2], [1, 0])), (([0, 1], [v, v]), ([0, 1], [2, 2])), (([v, 0], [v, v]), ([2, 0], [2, 2]))):
                        same(m.convert_batch(rec, rec_lens, src=sv, tgt=tv, mode=mode, noise_seed=5),
                             f.convert_batch(rec, rec_lens, src=sf, tgt=tf, mode=mode, noise_seed=5), ("convert", arith, mode, sv, tv))
                    for ns in (0.0, 1.0):
                        got = m.align_batch(rec, ids, rec_lens, speakers=[v, v], noise_scale=ns, mode=mode, noise_seed=5)
                        want = f.align_batch(rec, ids, rec_lens, speakers=[2, 2], noise_scale=ns, mode=mode, noise_seed=5)
                        for g, w in zip(got, want):
                            np.testing.assert_array_equal(g, w, err_msg=str(("align", arith, mode, ns)))
                        assert got[0].sum(1).tolist() == got[1].tolist() == [37, 25]


# ---- 5. order does not matter --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["tiny", "full"])
def test_voices_before_and_after_prepare_conversion_convert_alike(pkg, export_bytes, full_vc_bytes, which):
    data = export_bytes if which == "tiny" else full_vc_bytes
    hop = 8 if which == "tiny" else 256
    rec, rec_lens = signals([hop * 30, hop * 19], seed=8)
    outs = []
    for order in ("before", "after", "between"):
        with pkg.Model(data) as m:
            vecs = np.random.default_rng(3).standard_normal((3, m.speaker_embedding_size)).astype(np.float32)
            if order == "before":
                voices = m.add_voices(vecs)
                m.prepare_conversion()
            elif order == "after":
                m.prepare_conversion()
                voices = m.add_voices(vecs)
            else:
                voices = m.add_voices(vecs[:1])
                m.prepare_conversion()
                voices += m.add_voices(vecs[1:])
            assert voices == [m.num_speakers + k for k in range(3)]
            outs.append([m.convert_batch(rec, rec_lens, src=[voices[0], voices[2]], tgt=[voices[1], 0], noise_seed=2),
                         m.convert_batch(rec, rec_lens, src=[1, voices[1]], tgt=[voices[2], voices[0]], noise_seed=2)])
    for other in outs[1:]:
        for got, want in zip(other, outs[0]):
            same(got, want)
    assert not np.array_equal(outs[0][0][0][0], outs[0][1][0][0])


@pytest.mark.parametrize("which", ["tiny", "full"])
def test_a_growing_table_leaves_every_earlier_row_alone(pkg, export_bytes, full_vc_bytes, which):
    """1 + 1 + 70 voices: three growths of both tables. Before the third and after it: speaker -1, file speakers (all three of the tiny file; the first
    rows, a spread and the last two rows before the voices of the FULL file's 109) and both early voices, each as TTS speaker, as conversion source and as
    conversion target, in fp32 and f16; the first voice also across the second growth."""
    data = export_bytes if which == "tiny" else full_vc_bytes
    hop = 8 if which == "tiny" else 256
    with pkg.Model(data) as m:
        N, E = m.num_speakers, m.speaker_embedding_size
        rng = np.random.default_rng(17)
        m.prepare_conversion()
        w0 = m.weight_bytes
        first = m.add_voices(rng.standard_normal(E).astype(np.float32))
        w1 = m.weight_bytes
        file_spk = [0, 1, 2] if which == "tiny" else [0, 1, 31, 64, 90, N - 2, N - 1]

        def outputs(spk):
            B = len(spk)
            ids = pkg.synth_ids(B, 16, ids_seed=9)
            rec, rec_lens = signals([hop * (18 + b) for b in range(B)], seed=3)
            res = {}
            for arith in ("ARITH_F32", "ARITH_F16"):
                m.set_arith(getattr(pkg, arith))
                res[arith] = (tts(m, ids, spk), m.convert_batch(rec, rec_lens, src=spk, tgt=spk[::-1], noise_seed=4),
                              m.convert_batch(rec, rec_lens, src=spk[1:] + spk[:1], tgt=spk, noise_seed=4))
            m.set_arith(pkg.ARITH_F32)
            return res

        def check(after, before, what):
            for arith in before:
                for got, want in zip(after[arith], before[arith]):
                    same(got, want, (what, arith))

        early = [-1] + file_spk + first
        before_second = outputs(early)
        second = m.add_voices(rng.standard_normal(E).astype(np.float32))
        w2 = m.weight_bytes
        check(outputs(early), before_second, "second growth")
        spk = early + second
        before = outputs(spk)
        rest = m.add_voices(rng.standard_normal((70, E)).astype(np.float32))
        w3 = m.weight_bytes
        assert first + second + rest == list(range(N, N + 72)) and m.num_voices == 72
        assert w0 < w1 < w2 < w3  # the tables grew at every one of the three registrations (capacities 1, 2, 72 voices)
        check(outputs(spk), before, "third growth")
        # the 16-bit packs were made before the tables moved: a late voice that repeats the first one is the first one in f16 too
        again = m.add_voices(m.speaker_embedding(first[0]))
        m.set_arith(pkg.ARITH_F16)
        ids = pkg.synth_ids(len(spk), 16, ids_seed=9)
        same(tts(m, ids, [again[0] if s == first[0] else s for s in spk]), before["ARITH_F16"][0])
        m.set_arith(pkg.ARITH_F32)


# ---- 6. a mixed batch equals its rows ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["tiny", "full"])
def test_a_mixed_batch_equals_its_rows(pkg, export_bytes, full_spk_bytes, which):
    data = export_bytes if which == "tiny" else full_spk_bytes
    ids = pkg.synth_ids(6, 40, ids_seed=2)
    lens = np.array([40, 7, 33, 40, 1, 20], np.int32)
    with pkg.Model(data) as m:
        E = m.speaker_embedding_size
        va = m.add_voice_mix([0, 1], [0.7, 0.3])
        vb = m.add_voices(np.random.default_rng(5).standard_normal(E).astype(np.float32))[0]
        np.testing.assert_array_equal(m.speaker_embedding(va), (np.float32(0.7) * m.speaker_embedding(0) + np.float32(0.3) * m.speaker_embedding(1)).astype(np.float32))
        spk = np.array([-1, 1, va, vb, 0, va], np.int32)
        for mode in (0, 1):
            want = tts(m, ids, spk, lens, mode=mode)
            for b in range(6):
                one = tts(m, ids[b:b + 1, :lens[b]], spk[b:b + 1], mode=mode, noise_seed_offsets=[b])
                np.testing.assert_array_equal(one[0][0], want[0][b], err_msg=str((mode, b)))
                assert one[1][0] == want[1][b] and one[2][0] == want[2][b]
                np.testing.assert_array_equal(one[3][0], want[3][b, :lens[b]])
        want = tts(m, ids, spk, lens)
        assert len({want[0][b].tobytes() for b in (0, 1, 2, 3, 4)}) == 5
        # two batches in flight
        d1, d2 = np.zeros(ids.shape, np.int32), np.zeros(ids.shape, np.int32)
        m.submit_batch(ids, id_lengths=lens, noise_seed=7, speaker_ids=spk, durations_out=d1)
        m.submit_batch(ids[::-1].copy(), id_lengths=lens[::-1].copy(), noise_seed=7, speaker_ids=spk[::-1].copy(), noise_seed_offsets=np.arange(6)[::-1].copy(),
                       durations_out=d2)
        got1, got2 = m.wait(), m.wait()
        same(got1 + (d1,), want, "pipelined")
        same(([x for x in got2[0][::-1]], got2[1][::-1], got2[2][::-1], d2[::-1]), want, "pipelined, reversed")
        # windowed vocoder with a streaming sink
        chunks = {}
        got = tts(m, ids, spk, lens, vocoder_chunk_frames=9, on_chunk=lambda u, off, x: chunks.setdefault(u, []).append((off, x)) and False)
        same(got, want, "windowed")
        for b in range(6):
            np.testing.assert_array_equal(np.concatenate([x for _, x in sorted(chunks[b], key=lambda c: c[0])]), want[0][b])
        # frames only
        got = tts(m, ids, spk, lens, frames_only=True)
        for k in (1, 2, 3):
            np.testing.assert_array_equal(got[k], want[k])


# ---- 7. set_voice, clear_voices, the default speaker ---------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["tiny", "full"])
def test_set_voice_clear_voices_and_the_default_speaker(pkg, export_bytes, full_vc_bytes, which):
    data = export_bytes if which == "tiny" else full_vc_bytes
    hop = 8 if which == "tiny" else 256
    ids = pkg.synth_ids(1, 20, ids_seed=6)
    rec, rec_lens = signals([hop * 26], seed=7)
    with pkg.Model(data) as m:
        N, E = m.num_speakers, m.speaker_embedding_size
        rng = np.random.default_rng(8)
        a, b, c = (rng.standard_normal(E).astype(np.float32) for _ in range(3))
        va, vb = m.add_voices(np.stack([a, b]))
        m.prepare_conversion()  # (from here on set_voice rewrites the row of the posterior encoder's table too)
        others = (-1, 0, 1, N - 1, vb)

        def conversions(v):
            return [m.convert_batch(rec, rec_lens, src=v, tgt=1, noise_seed=3), m.convert_batch(rec, rec_lens, src=0, tgt=v, noise_seed=3),
                    m.align_batch(rec, ids[:, :9], rec_lens, speakers=v, noise_scale=1.0, noise_seed=3)]

        def same_conversions(got, want, what):
            same(got[0], want[0], (what, "as source"))
            same(got[1], want[1], (what, "as target"))
            for g, w in zip(got[2], want[2]):
                np.testing.assert_array_equal(g, w, err_msg=str((what, "alignment")))

        def differs(x, y):
            return x[0][0].size != y[0][0].size or not np.array_equal(x[0][0], y[0][0])

        base = {s: tts(m, ids, [s]) for s in others + (va,)}
        base_vc = {s: conversions(s) for s in (va, vb, 0)}
        m.set_voice(va, c)
        np.testing.assert_array_equal(m.speaker_embedding(va), c)
        changed = tts(m, ids, [va])
        changed_vc = conversions(va)
        assert differs(changed, base[va])
        assert differs(changed_vc[0], base_vc[va][0]), "conversion from the re-set voice still reads the old row of the posterior's table"
        assert differs(changed_vc[1], base_vc[va][1]), "conversion into the re-set voice still reads the old row"
        for s in others:
            same(tts(m, ids, [s]), base[s], s)
        for s in (vb, 0):
            same_conversions(conversions(s), base_vc[s], s)
        m.set_voice(va, a)
        same(tts(m, ids, [va]), base[va], "set back")
        same_conversions(conversions(va), base_vc[va], "set back")
        # the default speaker may be a voice: the reference entry points speak with it
        m.set_speaker(vb)
        assert m.speaker == vb
        same(tts(m, ids, None), base[vb], "default speaker")
        pkg.lib().vits_reference_noise_seed(1)
        with_voice = m.process_ids(ids[0])
        m.set_voice(vb, m.speaker_embedding(1))
        pkg.lib().vits_reference_noise_seed(1)
        as_one = m.process_ids(ids[0])
        m.set_speaker(1)
        pkg.lib().vits_reference_noise_seed(1)
        np.testing.assert_array_equal(as_one, m.process_ids(ids[0]))
        assert with_voice.size != as_one.size or not np.array_equal(with_voice, as_one)
        m.set_speaker(-1)
        m.clear_voices()
        assert m.num_voices == 0
        with pytest.raises(pkg.VitsError, match=r"outside \[-1, %d\)" % N):
            tts(m, ids, [va])
        assert m.add_voices(c) == [N]
        same(tts(m, ids, [N]), changed, "first id again")
        same(m.convert_batch(rec, rec_lens, src=N, tgt=1, noise_seed=3), changed_vc[0], "first id again, conversion")


# ---- 8. the same kernels -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["ARITH_F32", "ARITH_F16"])
@pytest.mark.parametrize("which", ["tiny", "full"])
def test_a_call_with_voices_queues_the_kernels_of_a_call_with_speakers(pkg, export_bytes, full_vc_bytes, which, arith):
    data = export_bytes if which == "tiny" else full_vc_bytes
    hop = 8 if which == "tiny" else 256
    ids = pkg.synth_ids(3, 30, ids_seed=1)
    rec, rec_lens = signals([hop * 21, hop * 30, hop * 9], seed=2)
    with pkg.Model(data) as m:
        m.set_arith(getattr(pkg, arith))
        N = m.num_speakers
        v = m.add_voices(np.random.default_rng(1).standard_normal((2, m.speaker_embedding_size)).astype(np.float32))
        m.prepare_conversion()

        def kernels(call):
            call()  # (warm: lazily built weight copies are not part of the comparison)
            m.prof_reset()
            m.prof_enable(True)
            call()
            m.prof_enable(False)
            return sorted((k["name"], k["calls"]) for k in m.prof_report()["kernels"])

        for spk_f, spk_v in (([N // 20, -1, N - 1], [v[0], -1, v[1]]), ([0, 1, 2], [v[0], 1, v[1]])):
            want = kernels(lambda: tts(m, ids, spk_f))
            assert len(want) > 10
            assert kernels(lambda: tts(m, ids, spk_v)) == want
            want = kernels(lambda: m.convert_batch(rec, rec_lens, src=spk_f, tgt=spk_f[::-1], noise_seed=1))
            assert kernels(lambda: m.convert_batch(rec, rec_lens, src=spk_v, tgt=spk_v[::-1], noise_seed=1)) == want
            want = kernels(lambda: m.align_batch(rec, ids[:, :8], rec_lens, speakers=spk_f))
            assert kernels(lambda: m.align_batch(rec, ids[:, :8], rec_lens, speakers=spk_v)) == want


# ---- 9. memory accounting and the embeddings -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["tiny", "full"])
def test_weight_bytes_and_embeddings(pkg, export_bytes, full_vc_bytes, which):
    data = export_bytes if which == "tiny" else full_vc_bytes
    tensors = parse_model_file(data)["tensors"]
    emb = tensors["embed_speaker.weight"][0]
    N, E = emb.shape
    # conditioned channels = rows of the conditioning convs the file holds ([rows, E, 1]): the resident weights and the row strides follow from them
    main = sum(t[0].shape[0] for name, t in tensors.items() if name in ("duration_predictor.cond.weight", "decoder.cond.weight") or
               (name.startswith("flow.flows.") and name.endswith(".wavenet.cond_layer.weight")))
    post = tensors["posterior_encoder.wavenet.cond_layer.weight"][0].shape[0]
    assert (N, E, main, post) == ((3, 8, 16 + 2 * 2 * 32 + 32, 32) if which == "tiny" else (109, 256, 6848, 16 * 384))
    ids = pkg.synth_ids(1, 12)
    with pkg.Model(data) as m:
        assert m.speaker_embedding_size == E and m.num_speakers == N
        w_load = m.weight_bytes
        tts(m, ids, [2])  # (the first small call makes the latency kernels' weight copy: counted before the comparison starts)
        w0 = m.weight_bytes
        tts(m, ids, [2])
        for s in (0, N // 2, N - 1):
            np.testing.assert_array_equal(m.speaker_embedding(s), emb[s].astype(np.float32))
        assert m.weight_bytes == w0  # a handle without voices allocates nothing
        vec = np.random.default_rng(2).standard_normal((2, E)).astype(np.float32)
        v = m.add_voices(vec)
        assert m.weight_bytes >= w0 + main * E * 4 + 2 * main * 4  # the resident cond convs (fp32) and two table rows
        w1 = m.weight_bytes
        m.prepare_conversion()
        w2 = m.weight_bytes
        with pkg.Model(data) as plain:
            p0 = plain.weight_bytes
            plain.prepare_conversion()
            # the posterior's table takes the two voices' rows and its cond conv becomes resident
            assert (w2 - w1) - (plain.weight_bytes - p0) >= post * E * 4 + 2 * post * 4
            assert p0 == w_load
        for k in range(2):
            np.testing.assert_array_equal(m.speaker_embedding(v[k]), vec[k])
        buf = np.full(300, -7.0, np.float32)
        assert pkg.lib().vits_model_get_speaker_embedding(m._h, v[1], buf.ctypes.data, 5) == E
        np.testing.assert_array_equal(buf[:5], vec[1, :5])
        assert (buf[5:] == -7.0).all()
    with pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_TINY)) as single:
        assert single.speaker_embedding_size == 0 and single.num_voices == 0


# ---- 10. refusals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["tiny", "full"])
def test_refusals_name_the_culprit_and_leave_the_handle_alone(pkg, export_bytes, full_vc_bytes, tiny_bytes, full_bytes, which):
    data = export_bytes if which == "tiny" else full_vc_bytes
    hop = 8 if which == "tiny" else 256
    ids = pkg.synth_ids(2, 14, ids_seed=8)
    rec, rec_lens = signals([hop * 20, hop * 30], seed=1)
    with pkg.Model(data) as m:
        N, E = m.num_speakers, m.speaker_embedding_size
        lim = r"outside \[-1, %d\)" % (N + 2)
        past = N + 2
        good = np.random.default_rng(4).standard_normal((2, E)).astype(np.float32)
        v = m.add_voices(good)
        assert v == [N, N + 1]
        m.prepare_conversion()  # (an alignment call would prepare it, and the first small call makes the latency kernels' weight copy: both before `w`)
        m.align_batch(rec, ids[:, :6], rec_lens, speakers=[v[1], 0])
        want = tts(m, ids, [v[0], v[1]])
        want_vc = m.convert_batch(rec, rec_lens, src=[v[0], 0], tgt=[1, v[1]], noise_seed=6)
        w = m.weight_bytes

        def unchanged(w=w):
            assert m.num_voices == 2 and m.weight_bytes == w and m.pending == 0
            same(tts(m, ids, [v[0], v[1]]), want)
            same(m.convert_batch(rec, rec_lens, src=[v[0], 0], tgt=[1, v[1]], noise_seed=6), want_vc)
            for k in range(2):
                np.testing.assert_array_equal(m.speaker_embedding(v[k]), good[k])

        with pytest.raises(pkg.VitsError, match="at least one"):
            m.add_voices(np.zeros((0, E), np.float32))
        out = np.zeros(2, np.int32)
        assert pkg.lib().vits_model_add_voices(m._h, good.ctypes.data, -3, out.ctypes.data) == -1 and "n = -3" in pkg.last_error()
        assert pkg.lib().vits_model_add_voices(m._h, None, 1, out.ctypes.data) == -1 and "null" in pkg.last_error()
        assert pkg.lib().vits_model_add_voices(m._h, good.ctypes.data, 1, None) == -1 and "null" in pkg.last_error()
        assert pkg.lib().vits_model_set_voice(m._h, v[0], None) == -1 and "null" in pkg.last_error()
        assert pkg.lib().vits_model_get_speaker_embedding(m._h, 0, None, 4) == -1 and "null" in pkg.last_error()
        unchanged()
        last = E - 1
        for bad_value in (np.nan, np.inf, -np.inf):
            bad = good.copy()
            bad[1, last] = bad_value
            with pytest.raises(pkg.VitsError, match=r"voice 1 \(id %d\), element %d is not finite" % (N + 3, last)):
                m.add_voices(bad)
            with pytest.raises(pkg.VitsError, match=r"voice 0 \(id %d\), element %d is not finite" % (v[1], last)):
                m.set_voice(v[1], bad[1])
        unchanged()
        for bad_id in (-1, 0, N - 1, past, 9999):
            with pytest.raises(pkg.VitsError, match=r"set_voice\(%d\): not a registered voice" % bad_id):
                m.set_voice(bad_id, good[0])
        for bad_id in (-1, past, 9999):
            with pytest.raises(pkg.VitsError, match=r"get_speaker_embedding\(%d\)" % bad_id):
                m.speaker_embedding(bad_id)
        unchanged()
        # an id past the registry stays refused everywhere, with the count of speakers and voices in the message
        with pytest.raises(pkg.VitsError, match=r"speaker_ids\[1\] = %d is %s" % (past, lim)):
            tts(m, ids, [v[0], past])
        with pytest.raises(pkg.VitsError, match=r"speaker_ids\[0\] = %d is %s" % (past, lim)):
            m.submit_batch(ids, speaker_ids=[past, 0])
        with pytest.raises(pkg.VitsError, match=r"set_speaker\(%d\): %s" % (past, lim)):
            m.set_speaker(past)
        with pytest.raises(pkg.VitsError, match=r"src_speakers\[1\] = %d .*%s" % (past, lim)):
            m.convert_batch(rec, rec_lens, src=[v[0], past], tgt=[0, 0])
        with pytest.raises(pkg.VitsError, match=r"tgt_speakers\[0\] = %d .*%s" % (past + 2, lim)):
            m.convert_batch(rec, rec_lens, src=[v[0], 0], tgt=[past + 2, 0])
        with pytest.raises(pkg.VitsError, match=r"speakers\[1\] = %d .*%s" % (past, lim)):
            m.align_batch(rec, ids[:, :6], rec_lens, speakers=[v[1], past])
        unchanged()
        # batches in flight
        m.submit_batch(ids, speaker_ids=[v[0], v[1]], noise_seed=7)
        for call in (lambda: m.add_voices(good), lambda: m.set_voice(v[0], good[1]), lambda: m.clear_voices()):
            with pytest.raises(pkg.VitsError, match="batches in flight"):
                call()
        got = m.wait()
        same(got, want[:3])
        unchanged()
        # from inside a callback
        seen = []

        def sink(utt, off, x):
            for call in (lambda: m.add_voices(good), lambda: m.set_voice(v[0], good[1]), lambda: m.clear_voices()):
                try:
                    call()
                    seen.append("accepted")
                except pkg.VitsError as e:
                    seen.append(str(e))
            return False

        same(tts(m, ids, [v[0], v[1]], vocoder_chunk_frames=16, on_chunk=sink), want)
        assert len(seen) >= 3 and all("model busy" in s for s in seen), seen
        unchanged()
        # the default speaker is a voice: the registry may not shrink under it
        m.set_speaker(v[1])
        with pytest.raises(pkg.VitsError, match=r"default speaker %d is a voice" % v[1]):
            m.clear_voices()
        m.set_speaker(-1)
        unchanged()
        # the exact-order stage one has no speaker conditioning: voices are refused as speakers are
        m.set_ggml_tables(1)  # (accepted: uploads the lookup tables and the exact-order tensors)
        w_tables = m.weight_bytes
        with pytest.raises(pkg.VitsError, match=r"speaker_ids\[1\] = %d.*set_ggml_tables" % v[1]):
            tts(m, ids, [-1, v[1]])
        m.set_ggml_tables(0)
        unchanged(w_tables)
    with pkg.Model(tiny_bytes if which == "tiny" else full_bytes) as single:
        want = tts(single, ids, [-1, -1])
        for call in (lambda: single.add_voices(np.zeros((1, 8), np.float32)), lambda: single.set_voice(1, np.zeros(8, np.float32)), lambda: single.clear_voices(),
                     lambda: single.speaker_embedding(0)):
            with pytest.raises(pkg.VitsError, match="single speaker"):
                call()
        assert single.num_voices == 0
        same(tts(single, ids, [-1, -1]), want)


# ---- against transformers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture,mode", [("tiny_speakers_hf_export_voices_taps.npz", 1), ("tiny_speakers_hf_export_voices_refmode_taps.npz", 0)])
def test_voices_match_transformers_taps(pkg, export_bytes, fixture, mode):
    """test_speakers_match_transformers_taps with voices: transformers ran with embed_speaker.weight[slot] overwritten by each vector; here the vector
    is a registered voice on the untouched file. The bound is that test's (2e-4 relative RMS). Durations are ceil() of a float, so their equality is
    demanded of inputs whose exp(log_duration) / speaking_rate stays at least `margin` (>= 0.02 frame, stored by the generator from transformers'
    own values) away from an integer."""
    g = golden(fixture)
    dec = int(g["decimate"][0])
    assert float(g["margin"][0]) >= 0.02
    with pkg.Model(export_bytes) as m:
        np.testing.assert_array_equal(g["vectors"][0], (np.float32(0.5) * m.speaker_embedding(0) + np.float32(0.5) * m.speaker_embedding(1)).astype(np.float32))
        voices = m.add_voices(g["vectors"])
        assert len(voices) == 3
        frames = set()
        for i, v in enumerate(voices):
            k = "v%d" % i
            pcm, lengths, _ = m.process_batch(g["ids"], mode=mode, noise_kind=pkg.NOISE_EXPLICIT, noise_dur=g["noise_dur"][None],
                                              noise_prior=g[k + "_noise_prior"][None], collect_taps=True, speaker_ids=[v])
            errs = {t: rel_err(m.tap(t), g[k + "_" + t]) for t in ("log_duration", "z_flow")}
            errs["waveform"] = rel_err(pcm[0][::dec], g[k + "_waveform"]) if lengths[0] == int(g[k + "_waveform_len"][0]) else None
            print(fixture, k, errs)
            np.testing.assert_array_equal(m.tap("durations"), g[k + "_durations"].ravel(), err_msg=k)
            assert errs["log_duration"] < 2e-4, k
            assert errs["z_flow"] < 2e-4, k
            assert lengths[0] == int(g[k + "_waveform_len"][0]), k
            assert errs["waveform"] < 2e-4, k
            frames.add(int(g[k + "_durations"].sum()))
        assert len(frames) > 1  # the fixture's voices really move the durations
