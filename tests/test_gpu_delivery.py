"""The delivery chain as a whole: every combination of the stages behind the vocoder (stated edges, level or limiter, output rate) through every way a
call hands its PCM out, against the operators chained on the plain call's waveforms (pkg.edges, then pkg.level or pkg.limit, then pkg.resample), bit
for bit: the PCM, lengths[], the rows of last_levels() / last_limits() / last_edges() (None where the stage is off), and nothing written past a row's
bound in a caller-owned buffer. Streaming tiles the non-streamed call; the refusals keep their texts; the first call with every stage on grows
vits_model_weight_bytes by what it always did.

The tiny model (16 kHz, hop 8), three ragged utterances at fixed_duration 60 (300, 720 and 1860 frames): the rows differ in length and the trimmed
lengths differ from the bounds, so a wrong stride, source or length shows. The operators run once per stage combination on the whole ragged batch."""
import numpy as np
import pytest

from delivery_helpers import FS, LENS, MARGIN, PADS, SHAPE, DeviceRows, choose, same
import edges_ref as ER

pytestmark = pytest.mark.gpu

FD = 60
RATE = 44100
LEVELS = ("none", "measure", "gain", "loudness", "gain+limiter", "loudness+limiter")
COMBOS = [(ed, lv, rate) for ed in (False, True) for lv in LEVELS for rate in (0, RATE)]
GAIN_DB = -3.0
SENTINEL = 7.25
# vits_model_weight_bytes of a fresh handle of the tiny model after its first call with edges, loudness, the limiter and 44100 Hz set: the value the
# engine of commit 3034c06 (the parent of the delivery-plan refactor) reports for the sequence of test_weight_bytes_after_the_first_call_with_every_stage
WEIGHT_BYTES_ALL_STAGES = 3551896


def call(m, ids, **kw):
    return m.process_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=FD, **kw)


@pytest.fixture(scope="module")
def ids(pkg):
    return pkg.synth_ids(3, 31)


@pytest.fixture(scope="module")
def tiny(pkg, tiny_bytes):
    with pkg.Model(tiny_bytes) as m:
        assert m.sampling_rate == FS and m.hop == 8
        yield m


@pytest.fixture(scope="module")
def split_model(pkg, tiny_bytes):
    """a handle of its own that splits batches of two or more inside the call (the knob is read when the model is loaded)"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("VITS_SPLIT_MIN_BATCH", "2")
        m = pkg.Model(tiny_bytes)
    with m:
        yield m


@pytest.fixture(scope="module")
def plain(tiny, ids):
    """the call with every stage off: (pcm, lengths, frames)"""
    configure_off(tiny)
    pcm, lengths, frames = call(tiny, ids)
    assert tiny.last_levels() is None and tiny.last_limits() is None and tiny.last_edges() is None
    assert frames.tolist() == [FD * int(n) for n in LENS]
    return pcm, lengths, frames


@pytest.fixture(scope="module")
def desc(pkg, plain):
    th = choose(plain[0])
    assert th is not None
    assert all(ER.margin(w, FS, ER.TRIM_RELATIVE, th, **SHAPE) >= MARGIN for w in plain[0])
    return dict(SHAPE, mode=pkg.EDGES_TRIM_RELATIVE, threshold_db=th)


def ragged(rows):
    """the rows side by side, zeros behind each: ([B][longest], lengths)"""
    n = np.array([r.size for r in rows], np.int64)
    x = np.zeros((len(rows), int(n.max())), np.float32)
    for b, r in enumerate(rows):
        x[b, :r.size] = r
    return x, n


class Refs:
    """the expected delivery of every stage combination, each stage of each chain computed once"""

    def __init__(self, pkg, plain, desc):
        self.pkg, self.desc = pkg, desc
        self.waves = {False: [w.copy() for w in plain[0]]}
        self.bound = {False: np.array([w.size for w in plain[0]], np.int64)}
        x, n = ragged(plain[0])
        y, n1, rows = pkg.edges(x, FS, lens=n, **desc)
        self.waves[True] = [y[b, :n1[b]].copy() for b in range(3)]
        self.bound[True] = self.bound[False] + PADS
        self.ed_rows = rows.copy()
        assert np.array_equal(rows[:, 2], n1) and (n1 < self.bound[True]).sum() >= 2  # the stage does trim here
        self.levelled, self.out = {}, {}

    def targets(self, ed):
        """(loudness target, ceiling): the loudness of utterance 2 under a ceiling 6 dB below its peak, so that the limiter works in earnest. At this
        duration the trimmed rows are all shorter than a gating block (0.4 s): unmeasurable, so levelling leaves them at gain 1 whatever the target, and
        the target is then the plain utterance's (0.93 s, six blocks); the ceiling is always taken from the row that is levelled."""
        y0 = self.waves[ed][2]
        value = float(np.float32(self.pkg.loudness_host(y0, FS)[0]))
        if not np.isfinite(value):
            value = float(np.float32(self.pkg.loudness_host(self.waves[False][2], FS)[0]))
        ceiling = float(np.float32(20.0 * np.log10(float(np.abs(y0).max())) - 6.0))
        assert -70 <= value <= 0 and -60 <= ceiling <= 0
        return value, ceiling

    def level_args(self, ed, lv):
        """(kind, value_db, ceiling_db, limiter on) as the handle is set for `lv`"""
        pkg = self.pkg
        value, ceiling = self.targets(ed)
        return {"none": (pkg.LEVEL_NONE, 0.0, 0.0, False), "measure": (pkg.LEVEL_MEASURE, 0.0, 0.0, False), "gain": (pkg.LEVEL_GAIN, GAIN_DB, 0.0, False),
                "loudness": (pkg.LEVEL_LOUDNESS, value, ceiling, False), "gain+limiter": (pkg.LEVEL_GAIN, GAIN_DB, ceiling, True),
                "loudness+limiter": (pkg.LEVEL_LOUDNESS, value, ceiling, True)}[lv]

    def level(self, ed, lv):
        """(rows at the model's rate, levels [3][4] or None, limits [3][4] or None)"""
        if (ed, lv) not in self.levelled:
            pkg = self.pkg
            kind, value, ceiling, lim = self.level_args(ed, lv)
            x, n = ragged(self.waves[ed])
            if kind == pkg.LEVEL_NONE:
                got = (self.waves[ed], None, None)
            elif kind == pkg.LEVEL_MEASURE:
                got = (self.waves[ed], pkg.level(x, FS, kind, lens=n, apply=False)[1], None)
            elif not lim:
                y, levels = pkg.level(x, FS, kind, value, ceiling, lens=n)
                got = ([y[b, :n[b]].copy() for b in range(3)], levels, None)
            else:
                y, levels, limits = pkg.limit(x, FS, kind, value, ceiling, lens=n)
                assert limits[2, 2] < 1.0  # the limiter does turn utterance 2 down
                got = ([y[b, :n[b]].copy() for b in range(3)], levels, limits)
            self.levelled[(ed, lv)] = got
        return self.levelled[(ed, lv)]

    def want(self, combo):
        """dict(pcm, lengths, bound, levels, limits, edges) of one combination"""
        ed, lv, rate = combo
        rows, levels, limits = self.level(ed, lv)
        bound = self.bound[ed]
        if rate:
            if combo not in self.out:
                x, n = ragged(rows)
                y, n_out = self.pkg.resample(x, FS, rate, lens=n)
                self.out[combo] = [y[b, :n_out[b]].copy() for b in range(3)]
            rows = self.out[combo]
            bound = np.array([self.pkg.resample_length(FS, rate, int(v)) for v in bound], np.int64)
        return dict(pcm=rows, lengths=np.array([r.size for r in rows], np.int64), bound=bound, levels=levels, limits=limits, edges=self.ed_rows if ed else None)


@pytest.fixture(scope="module")
def refs(pkg, plain, desc):
    return Refs(pkg, plain, desc)


def configure_off(m):
    m.set_rates(0, 0)
    m.set_level(0)
    m.set_limiter(0)
    m.set_edges(0)


def configure(pkg, m, refs, combo):
    ed, lv, rate = combo
    kind, value, ceiling, lim = refs.level_args(ed, lv)
    m.set_limiter(pkg.LIMIT_TRUE_PEAK if lim else pkg.LIMIT_OFF)  # (first: a gain keeps its ceiling only with the limiter on)
    m.set_level(kind, value, ceiling)
    m.set_edges(**refs.desc) if ed else m.set_edges(pkg.EDGES_OFF)
    m.set_rates(0, rate)


def rows_match(got, want):
    return (got is None and want is None) or (got is not None and want is not None and got.shape == want.shape and
                                             (same(got, want) if want.dtype == np.float32 else np.array_equal(got, want)))


def check(m, result, want, path, n=3):
    """the PCM, the lengths and the three reports of the first n utterances"""
    pcm, lengths, frames = result
    assert np.array_equal(lengths, want["lengths"][:n]), (path, lengths, want["lengths"])
    assert frames.tolist() == [FD * int(v) for v in LENS[:n]], path
    for b in range(n):
        assert same(pcm[b], want["pcm"][b]), (path, b)
    for name in ("levels", "limits", "edges"):
        got, w = getattr(m, "last_" + name)(), want[name]
        assert rows_match(got, None if w is None else w[:n]), (path, name, got, w)


@pytest.fixture()
def model(tiny):
    yield tiny
    configure_off(tiny)


@pytest.fixture()
def split(split_model):
    yield split_model
    configure_off(split_model)


@pytest.mark.parametrize("ed,lv,rate", COMBOS)
def test_every_path_delivers_the_chained_operators(pkg, model, split, ids, refs, ed, lv, rate):
    combo = (ed, lv, rate)
    want = refs.want(combo)
    assert (want["lengths"] <= want["bound"]).all() and (not ed or (want["lengths"] < want["bound"]).any())
    configure(pkg, model, refs, combo)
    # a synchronous host copy
    check(model, call(model, ids), want, "sync")
    # a caller-owned device buffer, rows a few columns wider than the longest bound, no host copy
    cap = int(want["bound"].max()) + 3
    with DeviceRows(3, cap) as dev:
        dev.fill(SENTINEL)
        none, lengths, frames = call(model, ids, out_device=dev.ptr, out_device_stride=cap, skip_host_copy=True)
        got = dev.read()
        assert none is None
        check(model, ([got[b, :lengths[b]] for b in range(3)], lengths, frames), want, "out_device")
        for b in range(3):
            assert (got[b, want["bound"][b]:] == SENTINEL).all(), ("written past the bound", b)
    # the pipeline: two batches in flight, each wait reports its own batch
    model.submit_batch(ids, id_lengths=LENS, noise_seed=7, fixed_duration=FD)
    model.submit_batch(ids[:2], id_lengths=LENS[:2], noise_seed=7, fixed_duration=FD)
    check(model, model.wait(), want, "submit / wait")
    check(model, model.wait(), want, "submit / wait, second batch", n=2)
    # vocoder windows without a sink: the stages run behind the last window
    check(model, call(model, ids, vocoder_chunk_frames=257), want, "windows")
    # the batch split in two inside the call
    configure(pkg, split, refs, combo)
    check(split, call(split, ids), want, "split")


@pytest.mark.parametrize("window", (8, 13))
@pytest.mark.parametrize("rate", (0, RATE))
@pytest.mark.parametrize("lv", ("none", "gain"))
def test_streamed_chunks_tile_the_delivered_utterance(pkg, model, ids, refs, lv, rate, window):
    combo = (False, lv, rate)
    want = refs.want(combo)
    configure(pkg, model, refs, combo)
    whole = call(model, ids)
    check(model, whole, want, "not streamed")
    chunks = {}
    streamed = call(model, ids, vocoder_chunk_frames=window, on_chunk=lambda u, off, x: chunks.setdefault(u, []).append((off, x)) and False)
    check(model, streamed, want, "streamed")
    for b in range(3):
        pos = 0
        for off, x in chunks[b]:
            assert off == pos and x.size > 0, (b, off, pos)
            pos += x.size
        assert pos == want["lengths"][b] and len(chunks[b]) > 1
        assert same(np.concatenate([x for _, x in chunks[b]]), whole[0][b]), b


def test_refusals_keep_their_texts(pkg, model, ids, refs):
    called = []
    sink = dict(vocoder_chunk_frames=13, on_chunk=lambda u, off, x: called.append(u) and False)
    value, ceiling = refs.targets(False)
    model.set_limiter(pkg.LIMIT_TRUE_PEAK)
    for kind in (pkg.LEVEL_GAIN, pkg.LEVEL_LOUDNESS):  # (with the limiter on, its refusal comes first)
        model.set_level(kind, value, ceiling)
        with pytest.raises(pkg.VitsError, match="limiter.*looks 80 samples ahead and 880 back.*halo"):
            call(model, ids, **sink)
    model.set_limiter(pkg.LIMIT_OFF)
    model.set_edges(**refs.desc)
    for kind in (pkg.LEVEL_MEASURE, pkg.LEVEL_PEAK, pkg.LEVEL_LOUDNESS):  # (with or without edges: the level's refusal comes before theirs)
        model.set_level(kind, value, ceiling)
        with pytest.raises(pkg.VitsError, match="needs the whole utterance.*only VITS_LEVEL_GAIN streams"):
            call(model, ids, **sink)
    for kind in (pkg.LEVEL_NONE, pkg.LEVEL_GAIN):
        model.set_level(kind, GAIN_DB)
        with pytest.raises(pkg.VitsError, match="on_chunk.*edges.*the end of the utterance decides"):
            call(model, ids, **sink)
        with pytest.raises(pkg.VitsError, match="async.*edges.*host read"):
            call(model, ids, skip_host_copy=True, async_=True)
    assert not called
    # the handle still delivers
    model.set_level(pkg.LEVEL_NONE)
    check(model, call(model, ids), refs.want((True, "none", 0)), "after the refusals")


def test_weight_bytes_after_the_first_call_with_every_stage(pkg, tiny_bytes, ids, refs):
    with pkg.Model(tiny_bytes) as m:
        before = m.weight_bytes
        configure(pkg, m, refs, (True, "loudness+limiter", RATE))
        assert m.weight_bytes == before  # (nothing is allocated by the setters)
        check(m, call(m, ids), refs.want((True, "loudness+limiter", RATE)), "fresh handle")
        print("weight_bytes:", before, "->", m.weight_bytes)
        assert m.weight_bytes == WEIGHT_BYTES_ALL_STAGES
        call(m, ids)
        assert m.weight_bytes == WEIGHT_BYTES_ALL_STAGES
