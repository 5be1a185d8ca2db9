"""The host side of vits_model_process_joined and vits_model_speak, on the CPU.

The assembly of vits_model_speak (vits.cpp_amd/csrc/join_host.cpp speak_plan: the text cut into spans, the spans tokenised, the ones with ids laid out as the
batch of one joined call) runs in tests/speak_plan_dump.cpp, linked with join_host.o ALONE, with a toy tokenizer of the model tokenizer's shape: a letter is
1 + its place in the alphabet, a blank lies around every id, anything else is unknown. The expectations below are written out by hand. The program also
runs under AddressSanitizer + UBSan. Then: the symbols, the mirror's argument types, and what the entry points refuse without a device."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vits.cpp_amd", "csrc")


def build(target):
    subprocess.check_call(["make", "-s", "-C", CSRC, target])
    return os.path.join(CSRC, target)


@pytest.fixture(scope="module", params=["speak_plan_dump", "_asan/speak_plan_dump"])
def dump(request):
    exe = build(request.param)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")

    def run(text, sentence=250, paragraph=800, per_paragraph=0):
        got = subprocess.run([exe, str(sentence), str(paragraph), str(per_paragraph), text], capture_output=True, env=env)
        assert got.returncode in (0, 1) and not got.stderr, got.stderr[-2000:]
        return got.returncode, got.stdout.decode()
    return run


def toy(word):
    ids = [0]
    for ch in word.lower():
        if "a" <= ch <= "z":
            ids += [ord(ch) - ord("a") + 1, 0]
    return ids


def table(spans, stride=None):
    """spans: (index, track, gap, text) -> the program's output"""
    rows = [(i, t, g, toy(w)) for i, t, g, w in spans]
    stride = stride or max(len(r[3]) for r in rows)
    out = ["batch %d id_stride %d" % (len(rows), stride)]
    for i, t, g, ids in rows:
        out.append("span %d track %d gap %g len %d ids %s" % (i, t, g, len(ids), ",".join(str(v) for v in ids + [0] * (stride - len(ids)))))
    return "\n".join(out) + "\n"


def test_three_sentences_of_one_line(dump):
    assert dump("wait... what?! ok") == (0, table([(0, 0, 0, "wait"), (1, 0, 250, "what"), (2, 0, 250, "ok")]))
    # (written out once in full: the blank-interleaved ids, zeros past a span's length)
    assert dump("wait... what?! ok")[1] == ("batch 3 id_stride 9\nspan 0 track 0 gap 0 len 9 ids 0,23,0,1,0,9,0,20,0\nspan 1 track 0 gap 250 len 9 ids 0,23,0,8,0,1,0,20,0\n"
                                            "span 2 track 0 gap 250 len 5 ids 0,15,0,11,0,0,0,0,0\n")


def test_two_paragraphs(dump):
    text = "One. Two.\n\nThree! Four"
    assert dump(text) == (0, table([(0, 0, 0, "one"), (1, 0, 250, "two"), (2, 0, 800, "three"), (3, 0, 250, "four")]))
    assert dump(text, per_paragraph=1) == (0, table([(0, 0, 0, "one"), (1, 0, 250, "two"), (2, 1, 800, "three"), (3, 1, 250, "four")]))
    # negative gaps (overlaps) travel as they are
    assert dump(text, sentence=-30, paragraph=-2000, per_paragraph=1) == (0, table([(0, 0, 0, "one"), (1, 0, -30, "two"), (2, 1, -2000, "three"), (3, 1, -30, "four")]))


def test_terminators_alone_are_no_span(dump):
    # the splitter reports no span for "?!" and "...": the indices are those of the spans it does report
    assert dump("Hi. ?! ... \n\n ... there") == (0, table([(0, 0, 0, "hi"), (1, 0, 800, "there")]))
    assert dump("... !! ?") == (1, "refused: no speakable span: the text holds 0 spans and none of them has a symbol the tokenizer knows\n")


def test_cjk_terminators(dump):
    text = "ab。cd！ef？gh"
    assert dump(text) == (0, table([(0, 0, 0, "ab"), (1, 0, 250, "cd"), (2, 0, 250, "ef"), (3, 0, 250, "gh")]))


def test_a_dropped_span_hands_its_paragraph_end_on(dump):
    # span 2 ("456", nothing the tokenizer knows) ends the first paragraph and is dropped: span 1 ends it then, and span 3 opens the next
    text = "One. Two. 456\n\nThree. 789"
    assert dump(text, per_paragraph=1) == (0, table([(0, 0, 0, "one"), (1, 0, 250, "two"), (3, 1, 800, "three")]))
    # a dropped span in the middle of a paragraph changes nothing around it; one at the very start has no span in front of it to hand anything to
    assert dump("One. 456. Two", per_paragraph=1) == (0, table([(0, 0, 0, "one"), (2, 0, 250, "two")]))
    assert dump("456\n\nOne. Two", per_paragraph=1) == (0, table([(1, 0, 0, "one"), (2, 0, 250, "two")]))
    # a paragraph of dropped spans alone: the paragraphs around it are still two
    assert dump("One.\n\n456. 789\n\nTwo", per_paragraph=1) == (0, table([(0, 0, 0, "one"), (3, 1, 800, "two")]))


@pytest.mark.parametrize("args,message", [
    (dict(text="--null"), "the text is NULL or empty"),
    (dict(text=""), "the text is NULL or empty"),
    (dict(text="123 456. 789"), "no speakable span: the text holds 2 spans and none of them has a symbol the tokenizer knows"),
    (dict(text="a. b", sentence=60001), "sentence_gap_ms = 60001: must be finite and in [-2000, 60000] ms"),
    (dict(text="a. b", paragraph=-2000.5), "paragraph_gap_ms = -2000.5: must be finite and in [-2000, 60000] ms"),
    (dict(text="a. b", sentence="nan"), "sentence_gap_ms = nan: must be finite and in [-2000, 60000] ms"),
    (dict(text="ok. a#b"), "the toy tokenizer refuses '#'"),
    (dict(text="ok. " + "ab" * 512), "span 1 (bytes 4 .. 1028) has 2049 ids, above the 2048 an utterance may have: break the sentence up"),
])
def test_what_the_assembly_refuses(dump, args, message):
    assert dump(**args) == (1, "refused: " + message + "\n")


def test_the_longest_span_that_is_taken(dump):
    rc, out = dump("ok. " + "ab" * 511 + "c")
    assert rc == 0 and out.startswith("batch 2 id_stride 2047\n")


def test_symbols_and_argument_types(pkg):
    L = pkg.lib()
    for name in ("vits_model_process_joined", "vits_model_last_joins", "vits_model_speak"):
        assert name in pkg.EXPORTED_SYMBOLS and hasattr(L, name)
    vp, i32 = C.c_void_p, C.c_int32
    assert L.vits_model_process_joined.argtypes == [vp, vp, vp, i32, i32, C.POINTER(pkg.ProcessOpts), vp, vp, C.POINTER(pkg.BatchResult)]
    assert L.vits_model_last_joins.argtypes == [vp, vp, C.c_size_t] and L.vits_model_last_joins.restype == C.c_int64
    assert L.vits_model_speak.argtypes == [vp, C.c_char_p, C.POINTER(pkg.SpeakOpts), C.POINTER(pkg.BatchResult)]
    # vits_speak_opts of include/vits.h: uint32, two floats, int32, a pointer
    assert [(n, t) for n, t in pkg.SpeakOpts._fields_] == [("struct_size", C.c_uint32), ("sentence_gap_ms", C.c_float), ("paragraph_gap_ms", C.c_float),
                                                          ("track_per_paragraph", C.c_int32), ("process", C.POINTER(pkg.ProcessOpts))]
    assert C.sizeof(pkg.SpeakOpts) == 24 and pkg.SpeakOpts.process.offset == 16
    # the mirror takes process_batch's keywords
    batch_kw = set(inspect.signature(pkg.Model.process_batch).parameters) - {"self", "ids", "id_lengths", "keep_pcm"}
    assert set(inspect.signature(pkg.Model._joined_opts).parameters) - {"B", "stride"} == batch_kw
    assert list(inspect.signature(pkg.Model.process_joined).parameters)[:5] == ["self", "ids", "id_lengths", "track", "gap_ms"]
    assert list(inspect.signature(pkg.Model.speak).parameters)[:5] == ["self", "text", "sentence_gap_ms", "paragraph_gap_ms", "track_per_paragraph"]
    assert callable(pkg.Model.last_joins)


def test_refusals_without_a_device(pkg):
    L = pkg.lib()
    res = pkg.BatchResult()
    ids = np.zeros(3, np.int32)
    assert L.vits_model_process_joined(None, ids.ctypes.data_as(C.c_void_p), None, 1, 3, None, None, None, C.byref(res)) == -1
    assert pkg.last_error() == "vits_model_process_joined: null argument"
    assert L.vits_model_speak(None, b"hello", None, C.byref(res)) == -1
    assert pkg.last_error() == "vits_model_speak: null argument (model)"
    assert L.vits_model_last_joins(None, None, 0) == -1
    assert not res.data and not res.lengths and res.batch == 0
