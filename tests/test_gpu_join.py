"""vits_model_process_joined and vits_model_speak: a batch joined into tracks inside the call, in front of the handle's level, limiter and resampler.

The reference is the chain a caller had to run before the call existed, every link of it an operator with tests of its own: process_batch on a handle with
only the edges stage set (its rows, lengths and last_edges), pkg.join on those rows, pkg.level or pkg.limit on the tracks, pkg.resample on the result. The
engine must equal it bit for bit: PCM, lengths, frames, and the four reports.

The tiny model (16 kHz, hop 8), five ragged utterances [5, 12, 31, 1, 8] ids at fixed_duration 20 (100 .. 620 frames): shorter than a gating block each,
longer than one together. Gaps [0, 250, -30, 0, -2000] ms: a pause, an overlap, a plain seam and an overlap the half rule clamps (to half of the one-id
utterance). Partitions: two tracks, one track, every utterance its own."""
import itertools

import numpy as np
import pytest

from delivery_helpers import FS, MARGIN, SHAPE, DeviceRows, choose, same
import edges_ref as ER
import loudness_ref as LR

pytestmark = pytest.mark.gpu

LENS = np.array([5, 12, 31, 1, 8], np.int32)
B = 5
FD = 20
GAPS = np.array([0, 250, -30, 0, -2000], np.float32)
PARTS = {"two": [0, 0, 0, 1, 1], "one": [0, 0, 0, 0, 0], "own": [0, 1, 2, 3, 4]}
EDGES = ("off", "pad", "trim")
LEVELS = ("none", "gain", "loudness", "peak+limiter")
RATES = (0, 8000, 44100)
SENTINEL = 7.25
SEED = 7
# every (edges, level) pair once, the rate and the partition rotating, then eight more so that every rate meets every edges mode and every level
_pairs = list(itertools.product(EDGES, LEVELS))
COMBOS = [(ed, lv, RATES[i % 3], list(PARTS)[(i // 3) % 3]) for i, (ed, lv) in enumerate(_pairs)]
COMBOS += [(ed, lv, RATES[(i + 1) % 3], list(PARTS)[(i + 1) % 3]) for i, (ed, lv) in enumerate(_pairs) if i % 3 != 1]
assert len(COMBOS) == 20 and len(set(COMBOS)) == 20


def tracks_of(part):
    t = np.asarray(PARTS[part])
    return [np.flatnonzero(t == g) for g in range(int(t.max()) + 1)]


def ragged(rows):
    n = np.array([r.size for r in rows], np.int64)
    x = np.zeros((len(rows), max(int(n.max()), 1)), np.float32)
    for b, r in enumerate(rows):
        x[b, : r.size] = r
    return x, n


def configure_off(m):
    m.set_rates(0, 0)
    m.set_level(0)
    m.set_limiter(0)
    m.set_edges(0)


@pytest.fixture(scope="module")
def ids(pkg):
    return pkg.synth_ids(B, 31)


@pytest.fixture(scope="module")
def tiny(pkg, tiny_bytes):
    with pkg.Model(tiny_bytes) as m:
        assert m.sampling_rate == FS and m.hop == 8
        yield m


@pytest.fixture()
def model(pkg, tiny):
    yield tiny
    configure_off(tiny)
    tiny.set_arith(pkg.ARITH_F32)


def batch(m, ids, **kw):
    kw.setdefault("fixed_duration", FD)
    return m.process_batch(ids, id_lengths=LENS, noise_seed=SEED, **kw)


def joined(m, ids, part, gaps=GAPS, **kw):
    kw.setdefault("fixed_duration", FD)
    return m.process_joined(ids, id_lengths=LENS, track=PARTS[part], gap_ms=gaps, noise_seed=SEED, **kw)


class Chain:
    """the chained operators, every link computed once per (arithmetic, edges mode, partition, level, rate)"""

    def __init__(self, pkg, m, ids):
        self.pkg, self.m, self.ids = pkg, m, ids
        self.cache = {}
        self.th = None

    def edges_desc(self, ed):
        pkg = self.pkg
        if ed == "off":
            return None
        if ed == "pad":
            return dict(SHAPE, mode=pkg.EDGES_PAD)
        if self.th is None:
            configure_off(self.m)
            waves = batch(self.m, self.ids)[0]
            self.th = choose(waves)
            assert self.th is not None
            assert all(ER.margin(w, FS, ER.TRIM_RELATIVE, self.th, **SHAPE) >= MARGIN for w in waves)
        return dict(SHAPE, mode=pkg.EDGES_TRIM_RELATIVE, threshold_db=self.th)

    def level_args(self, lv):
        pkg = self.pkg
        return {"none": (pkg.LEVEL_NONE, 0.0, 0.0, False), "gain": (pkg.LEVEL_GAIN, -3.0, 0.0, False), "loudness": (pkg.LEVEL_LOUDNESS, -23.0, -1.0, False),
                "peak+limiter": (pkg.LEVEL_PEAK, -3.0, 0.0, True)}[lv]

    def utterances(self, arith, ed):
        """process_batch on the handle with edges only: (rows, frames, last_edges, bounds)"""
        key = ("utt", arith, ed)
        if key not in self.cache:
            m = self.m
            configure_off(m)
            m.set_arith(arith)
            d = self.edges_desc(ed)
            if d:
                m.set_edges(**d)
            pcm, lengths, frames = batch(m, self.ids)
            ed_rows = m.last_edges()
            _, bound, _ = batch(m, self.ids, frames_only=True)
            assert (lengths <= bound).all() and frames.tolist() == [FD * int(n) for n in LENS]
            self.cache[key] = ([w.copy() for w in pcm], frames.copy(), ed_rows, bound.copy())
        return self.cache[key]

    def tracks(self, arith, ed, part, gaps=GAPS):
        """... then pkg.join: (tracks [T_g], rows [B][2], bounds [G])"""
        key = ("join", arith, ed, part, tuple(np.asarray(gaps).tolist()))
        if key not in self.cache:
            rows, _, _, bound = self.utterances(arith, ed)
            x, n = ragged(rows)
            y, tl, on = self.pkg.join(x, FS, lens=n, track=PARTS[part], gap_ms=gaps)
            _, bounds, _ = self.pkg.join_plan(FS, bound, PARTS[part], gaps)
            assert (tl <= bounds).all()
            self.cache[key] = ([y[g, : tl[g]].copy() for g in range(len(tl))], on.copy(), bounds.copy())
        return self.cache[key]

    def want(self, arith, ed, lv, rate, part):
        key = ("want", arith, ed, lv, rate, part)
        if key in self.cache:
            return self.cache[key]
        pkg = self.pkg
        _, frames, ed_rows, _ = self.utterances(arith, ed)
        rows, on, bounds = self.tracks(arith, ed, part)
        kind, value, ceiling, lim = self.level_args(lv)
        x, n = ragged(rows)
        levels = limits = None
        if lim:
            y, levels, limits = pkg.limit(x, FS, kind, value, ceiling, lens=n)
            rows = [y[g, : n[g]].copy() for g in range(len(n))]
        elif kind != pkg.LEVEL_NONE:
            y, levels = pkg.level(x, FS, kind, value, ceiling, lens=n)
            rows = [y[g, : n[g]].copy() for g in range(len(n))]
        if rate:
            x, n = ragged(rows)
            y, n_out = pkg.resample(x, FS, rate, lens=n)
            rows = [y[g, : n_out[g]].copy() for g in range(len(n))]
            bounds = np.array([pkg.resample_length(FS, rate, int(v)) for v in bounds], np.int64)
        joins = np.stack([np.arange(B), np.asarray(PARTS[part]), on[:, 0], on[:, 1]], axis=1).astype(np.int64)
        w = dict(pcm=rows, lengths=np.array([r.size for r in rows], np.int64), frames=np.array([frames[t].sum() for t in tracks_of(part)], np.int64),
                 bound=bounds, levels=levels, limits=limits, edges=ed_rows, joins=joins, join_last=kind == pkg.LEVEL_NONE and not rate)
        self.cache[key] = w
        return w

    def configure(self, arith, ed, lv, rate):
        pkg, m = self.pkg, self.m
        kind, value, ceiling, lim = self.level_args(lv)
        m.set_arith(arith)
        m.set_limiter(pkg.LIMIT_TRUE_PEAK if lim else pkg.LIMIT_OFF)
        m.set_level(kind, value, ceiling)
        d = self.edges_desc(ed)
        m.set_edges(**d) if d else m.set_edges(pkg.EDGES_OFF)
        m.set_rates(0, rate)


@pytest.fixture(scope="module")
def chain(pkg, tiny, ids):
    return Chain(pkg, tiny, ids)


def rows_match(got, want):
    return (got is None and want is None) or (got is not None and want is not None and got.shape == want.shape and
                                             (same(got, want) if want.dtype == np.float32 else np.array_equal(got, want)))


def check(m, result, want, path):
    pcm, lengths, frames = result
    G = len(want["pcm"])
    assert np.array_equal(lengths, want["lengths"]), (path, lengths, want["lengths"])
    assert np.array_equal(frames, want["frames"]), (path, frames, want["frames"])
    assert len(pcm) == G
    for g in range(G):
        assert same(pcm[g], want["pcm"][g]), (path, g)
    for name in ("levels", "limits", "edges", "joins"):
        got, w = getattr(m, "last_" + name)(), want[name]
        assert rows_match(got, w), (path, name, got, w)


def every_path(m, ids, part, want, tag):
    G = len(want["pcm"])
    check(m, joined(m, ids, part), want, tag + "host copy")
    # frames_only: per track the bound a full call stays within, and the summed frames
    none, bound, frames = joined(m, ids, part, frames_only=True)
    assert none is None and np.array_equal(bound, want["bound"]) and np.array_equal(frames, want["frames"]), (tag, bound, want["bound"])
    assert (want["lengths"] <= bound).all()
    cap = int(bound.max()) + 3
    with DeviceRows(G, cap) as dev:
        dev.fill(SENTINEL)
        none, lengths, frames = joined(m, ids, part, out_device=dev.ptr, out_device_stride=cap, skip_host_copy=True)
        got = dev.read()
        assert none is None
        check(m, ([got[g, : lengths[g]] for g in range(G)], lengths, frames), want, tag + "out_device")
        for g in range(G):
            assert (got[g, bound[g]:] == SENTINEL).all(), (tag, "written behind the bound", g)
            if want["join_last"]:
                tail = got[g, lengths[g]: bound[g]]
                assert not tail.any() and not np.signbit(tail).any(), (tag, "[T, bound) is not +0", g)
    check(m, joined(m, ids, part, vocoder_chunk_frames=8), want, tag + "windows")


@pytest.mark.parametrize("ed,lv,rate,part", COMBOS)
def test_the_engine_equals_the_chained_operators(pkg, model, ids, chain, ed, lv, rate, part):
    want = chain.want(pkg.ARITH_F32, ed, lv, rate, part)
    chain.configure(pkg.ARITH_F32, ed, lv, rate)
    every_path(model, ids, part, want, "%s %s %d %s: " % (ed, lv, rate, part))


def test_the_engine_equals_the_chain_in_f16(pkg, model, ids, chain):
    ed, lv, rate, part = "trim", "loudness", 44100, "two"
    want = chain.want(pkg.ARITH_F16, ed, lv, rate, part)
    assert not same(want["pcm"][0], chain.want(pkg.ARITH_F32, ed, lv, rate, part)["pcm"][0])  # (the mode does run)
    chain.configure(pkg.ARITH_F16, ed, lv, rate)
    every_path(model, ids, part, want, "f16: ")


def test_a_seam_on_a_tile_boundary(pkg, model, ids):
    """a zero-gap pair whose seam falls on a multiple of the join kernel's tile: fixed_duration places it"""
    tile = pkg.join_plan(FS, [1])[2]
    configure_off(model)
    found = None
    for mode in (pkg.MODE_HF, pkg.MODE_REFERENCE):
        _, n1, f1 = model.process_batch(ids[:1, :1], mode=mode, fixed_duration=1, frames_only=True)
        add = int(n1[0]) - 8 * int(f1[0])  # samples = hop * frames + add
        for t, fd in itertools.product(range(1, 32), range(1, 65)):
            if (8 * fd * t + add) % tile == 0:
                found = found or (mode, t, fd)
    assert found, "no (mode, ids, fixed_duration) puts an utterance's end on a tile boundary"
    mode, t, fd = found
    lens = np.array([t, 7], np.int32)
    pcm, lengths, _ = model.process_batch(ids[:2], id_lengths=lens, mode=mode, noise_seed=SEED, fixed_duration=fd)
    assert lengths[0] % tile == 0
    got, glen, _ = model.process_joined(ids[:2], id_lengths=lens, mode=mode, noise_seed=SEED, fixed_duration=fd)
    assert glen.tolist() == [int(lengths.sum())] and same(got[0], np.concatenate(pcm))
    assert model.last_joins().tolist() == [[0, 0, 0, int(lengths[0])], [1, 0, int(lengths[0]), int(lengths[1])]]


@pytest.mark.parametrize("ed,lv,rate", [("trim", "loudness", 44100), ("pad", "peak+limiter", 8000), ("off", "gain", 0)])
def test_every_utterance_its_own_track_is_the_plain_call(pkg, model, ids, chain, ed, lv, rate):
    chain.configure(pkg.ARITH_F32, ed, lv, rate)
    pcm, lengths, frames = batch(model, ids)
    reports = [getattr(model, "last_" + n)() for n in ("levels", "limits", "edges")]
    assert model.last_joins() is None
    got, glen, gframes = joined(model, ids, "own", gaps=None)
    assert np.array_equal(glen, lengths) and np.array_equal(gframes, frames)
    for b in range(B):
        assert same(got[b], pcm[b]), b
    for name, w in zip(("levels", "limits", "edges"), reports):
        assert rows_match(getattr(model, "last_" + name)(), w), name
    j = model.last_joins()
    assert np.array_equal(j[:, 0], np.arange(B)) and np.array_equal(j[:, 1], np.arange(B)) and not j[:, 2].any()


def test_the_programme_is_what_is_measured(pkg, model, ids, chain):
    rows, _, _, _ = chain.utterances(pkg.ARITH_F32, "off")
    tracks, _, _ = chain.tracks(pkg.ARITH_F32, "off", "one")
    alone = [LR.loudness(w, FS) for w in rows]
    whole = LR.loudness(tracks[0], FS)
    print("alone:", alone, "track:", whole)
    # the reference first: no utterance holds a 400 ms block, the track does
    assert all(w.size < 0.4 * FS for w in rows) and not any(np.isfinite(a[0]) for a in alone) and all(a[2] == 0 for a in alone)
    assert tracks[0].size >= 0.4 * FS and np.isfinite(whole[0]) and whole[2] > 0
    model.set_level(pkg.LEVEL_LOUDNESS, -23.0, -1.0)
    batch(model, ids)
    assert not np.isfinite(model.last_levels()[:, 0]).any()  # per utterance: nothing to measure
    joined(model, ids, "one")
    got = model.last_levels()
    want = chain.want(pkg.ARITH_F32, "off", "loudness", 0, "one")["levels"]
    assert got.shape == (1, 4) and np.isfinite(got[0, 0]) and same(got, want)


def plain_bits(m, ids):
    configure_off(m)
    return batch(m, ids, fixed_duration=0)


def submits(m, ids):
    m.submit_batch(ids, id_lengths=LENS, noise_seed=SEED)
    m.submit_batch(ids[:2], id_lengths=LENS[:2], noise_seed=SEED + 1)
    return [m.wait(), m.wait()]


def same_result(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and all(same(x, y) for x, y in zip(a[0], b[0]))


def test_refusals(pkg, model, tiny_bytes, ids):
    before = plain_bits(model, ids)
    sink = lambda u, off, x: False
    cases = [
        (dict(vocoder_chunk_frames=8, on_chunk=sink), r"vits_model_process_joined: on_chunk streams an utterance"),
        (dict(skip_host_copy=True, async_=True), r"vits_model_process_joined: async returns before the device has finished"),
        (dict(collect_taps=True), r"vits_model_process_joined: opts\.collect_taps is not taken.*per utterance.*per track"),
        (dict(noise_kind=pkg.NOISE_REFERENCE), r"vits_model_process_joined: noise_kind \d+ is not taken"),
    ]
    for kw, text in cases:
        with pytest.raises(pkg.VitsError, match=text):
            joined(model, ids, "two", **kw)
        assert same_result(plain_bits(model, ids), before), text
    for track, gaps, text in (([1, 1, 1, 2, 2], GAPS, r"vits_model_process_joined: track\[0\] = 1"), ([0, 0, 2, 2, 2], GAPS, r"vits_model_process_joined: track\[2\] = 2 after"),
                              (PARTS["two"], [0, 70000, 0, 0, 0], r"vits_model_process_joined: gap_ms\[1\] = 70000"),
                              (PARTS["two"], [0, 0, np.nan, 0, 0], r"vits_model_process_joined: gap_ms\[2\]")):
        with pytest.raises(pkg.VitsError, match=text):
            model.process_joined(ids, id_lengths=LENS, track=track, gap_ms=gaps, noise_seed=SEED, fixed_duration=FD)
        assert same_result(plain_bits(model, ids), before), text
    # batches in flight
    model.submit_batch(ids, id_lengths=LENS, noise_seed=SEED)
    with pytest.raises(pkg.VitsError, match="batches in flight"):
        joined(model, ids, "two")
    assert same_result(model.wait(), before)
    assert same_result(plain_bits(model, ids), before)
    # the two late refusals: a caller buffer one sample too small, with predicted durations (refused behind the frame-count read, before stage two is queued)
    # and with fixed_duration (refused before anything is queued); each followed once by two submits, which must give what a fresh handle gives
    with pkg.Model(tiny_bytes) as fresh:
        want = submits(fresh, ids)
    for fd in (0, FD):
        _, bound, _ = joined(model, ids, "two", frames_only=True, fixed_duration=fd)
        g = int(np.argmax(bound))
        cap = int(bound.max()) - 1
        with DeviceRows(2, cap) as dev:
            dev.fill(SENTINEL)
            with pytest.raises(pkg.VitsError, match=r"vits_model_process_joined: out_device_stride = %d is below track %d's %d samples" % (cap, g, cap + 1)):
                joined(model, ids, "two", fixed_duration=fd, out_device=dev.ptr, out_device_stride=cap, skip_host_copy=True)
            assert (dev.read() == SENTINEL).all()
        got = submits(model, ids)
        assert same_result(got[0], want[0]) and same_result(got[1], want[1]), fd
        assert same_result(plain_bits(model, ids), before), fd
    # the plain call's own late refusal drains the handle too
    with DeviceRows(B, 8) as dev:
        with pytest.raises(pkg.VitsError, match="out_device_stride is smaller than the longest utterance"):
            batch(model, ids, out_device=dev.ptr, out_device_stride=8, skip_host_copy=True)
    got = submits(model, ids)
    assert same_result(got[0], want[0]) and same_result(got[1], want[1])


def test_speak_is_process_joined_on_the_spans(pkg, model, ids):
    text = "wait... what?! ok\n\n%%%.\n\nhello there. a"
    spans = pkg.split_sentences(text)
    raw = text.encode("utf-8")
    toks = [model.tokenize(raw[s:e].decode("utf-8")) for s, e, _ in spans]
    assert [k for _, _, k in spans] == [0, 0, 1, 1, 0, 0] and [t.size > 1 for t in toks] == [True, True, True, False, True, True]
    keep = [i for i, t in enumerate(toks) if t.size > 1]
    stride = max(toks[i].size for i in keep)
    mat = np.zeros((len(keep), stride), np.int32)
    for r, i in enumerate(keep):
        mat[r, : toks[i].size] = toks[i]
    lens = np.array([toks[i].size for i in keep], np.int32)
    model.set_level(pkg.LEVEL_LOUDNESS, -23.0, -1.0)
    model.set_rates(0, 8000)
    for per_paragraph, track in ((False, [0, 0, 0, 0, 0]), (True, [0, 0, 0, 1, 1])):
        want = model.process_joined(mat, id_lengths=lens, track=track, gap_ms=[0, 120, 120, 400, 120], noise_seed=11)
        want_joins, want_levels = model.last_joins(), model.last_levels()
        got = model.speak(text, sentence_gap_ms=120, paragraph_gap_ms=400, track_per_paragraph=per_paragraph, noise_seed=11)
        assert same_result(got, want) and len(got[0]) == (2 if per_paragraph else 1)
        j = model.last_joins()
        assert j[:, 0].tolist() == keep and np.array_equal(j[:, 1:], want_joins[:, 1:]) and same(model.last_levels(), want_levels)
    for bad, text_re in ((dict(text=""), "vits_model_speak: the text is NULL or empty"), (dict(text="%%%...!"), "vits_model_speak: no speakable span"),
                         (dict(text="a. b", speaker_ids=[-1]), "vits_model_speak: process->speaker_ids is a per-utterance array"),
                         (dict(text="a. b", sentence_gap_ms=-2500), "vits_model_speak: sentence_gap_ms = -2500"),
                         (dict(text="a " * 1100), r"vits_model_speak: span 0 \(bytes 0 \.\. 2199\) has \d+ ids, above the 2048")):
        with pytest.raises(pkg.VitsError, match=text_re):
            model.speak(**bad)
