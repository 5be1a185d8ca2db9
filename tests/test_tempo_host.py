"""A stated tempo on the CPU (include/vits.h "a stated tempo"): the product's host-only pieces — vits_tempo_plan, vits_tempo_host — against the numpy
restatement (tests/tempo_ref.py) bit for bit; what the definition does to harmonic tones, measured on the product's host evaluation; the tempo half of the
delivery planner against its frozen table; and both host pieces as stand-alone programs under AddressSanitizer + UBSan.

tests/delivery_plan_dump.cpp (its slice `tempo`) links delivery_plan.o ALONE, walks every combination of the ask with tempo = true, with pitch and without, and prints one line per
case; the output must equal tests/golden/tempo_plan_table.txt byte for byte. The table was recorded once and is read line by line against the rules the last
test states; the test never regenerates it. The tables of the asks without tempo are tests/test_delivery_plan_host.py's, tests/test_joined_plan_host.py's and
tests/test_pitch_host.py's, which this stage leaves as they were."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import tempo_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vits.cpp_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "tempo_plan_table.txt")


def test_plan_is_the_restatement(pkg):
    for rate in (8000, 16000, 22050, 24000, 44100, 48000):
        for q in TR.TEMPOS:
            for n in (0, 1, 2, 159, 160, 161, 1000, 16001, 1 << 30):
                assert pkg.tempo_plan(rate, q, n) == TR.plan(rate, q, n), (rate, q, n)
    assert pkg.tempo_plan(16000, 1.0, 1000)[:3] == (160, 128, 1 << 24) and pkg.tempo_plan(22050, 1.0, 0)[:2] == (220, 176)
    assert pkg.tempo_plan(16000, 2.0, 1001)[3:] == (4, 501) and pkg.tempo_plan(16000, 0.5, 1001)[3:] == (13, 2002)
    for bad in (float("nan"), float("inf"), float(np.nextafter(np.float32(0.5), np.float32(0))), float(np.nextafter(np.float32(2), np.float32(3))), 0.0, -1.0):
        with pytest.raises(pkg.VitsError, match=r"not finite or outside \[0.5, 2\]"):
            pkg.tempo_plan(16000, bad, 10)
    for n in (-1, (1 << 30) + 1):
        with pytest.raises(pkg.VitsError, match=r"outside \[0, 2\^30\]"):
            pkg.tempo_plan(16000, 1.5, n)
    for rate in (7999, 48001, 0, -16000):
        with pytest.raises(pkg.VitsError, match=r"outside \[8000, 48000\]"):
            pkg.tempo_plan(rate, 1.5, 10)
    with pytest.raises(pkg.VitsError, match=r"outside \[8000, 48000\]"):
        pkg.tempo_host(np.zeros(10, np.float32), 7999, 1.5)
    with pytest.raises(pkg.VitsError, match=r"not finite or outside \[0.5, 2\]"):
        pkg.tempo_host(np.zeros(10, np.float32), 16000, 2.5)


@pytest.mark.parametrize("rate", TR.RATES)
@pytest.mark.parametrize("kind", TR.KINDS)
def test_host_evaluation_is_the_restatement_bit_for_bit(pkg, rate, kind):
    """offsets as integers, samples as uint32 views, every length and every tempo"""
    moved = 0
    for q in TR.TEMPOS:
        for n in TR.lengths(rate):
            x = TR.signal(kind, n)
            y, off = pkg.tempo_host(x, rate, q)
            want, want_off = TR.tempo(x, rate, q)
            H, D, Q, F, n_out = TR.plan(rate, q, n)
            assert y.size == want.size == n_out and off.size == want_off.size == F, (q, n)
            assert np.array_equal(off, want_off), (q, n, off, want_off)
            assert np.array_equal(y.view(np.uint32), want.view(np.uint32)), (q, n)
            assert (np.abs(off) <= D).all()
            moved += int(np.count_nonzero(off))
            if kind == "silence":
                assert not off.any() and not y.any()
            if Q == TR.ONE:
                assert np.array_equal(y.view(np.uint32), x.view(np.uint32)) and not off.any()
    # (a search that always answered 0 would pass the silent rows alone)
    assert (moved > 0) == (kind != "silence")


def test_ties_go_to_the_first_candidate_in_the_order(pkg):
    """a row of period 40 whose samples are multiples of 2^-15: candidates 40 apart have EQUAL sums, and the order 0, -1, +1, ... picks among them. Away from the
    row's ends every offset therefore lies within half a period of 0, and the negative one of a pair wins"""
    x = TR.signal("ties", 4000)
    xq = TR.quantise(x)
    assert np.array_equal(xq[:-40], xq[40:]) and np.array_equal(xq.astype(np.float32) / np.float32(32768), x)
    for q in (0.75, 1.25, 1.5):
        _, off = pkg.tempo_host(x, 16000, q)
        _, want = TR.tempo(x, 16000, q)
        assert np.array_equal(off, want)
        inner = off[2:-4]
        assert inner.size > 5 and (np.abs(inner) <= 20).all(), (q, off)
    # |d| = 20 has an equal partner at the other sign: the negative one is first in the order. A period of 2 makes every step such a pair
    x2 = np.tile(np.asarray([0.25, -0.25], np.float32), 2000)
    _, off = pkg.tempo_host(x2, 16000, 1.0 + 2.0 ** -8)
    assert set(off[2:-4].tolist()) <= {0, -1}, off


F0S = (83, 110, 233, 311)
TONE_TEMPOS = (0.5, 2.0 ** (-1 / 3), 2.0 ** (1 / 3), 2.0)


@pytest.mark.parametrize("f0", F0S)
def test_harmonic_tones_stay_harmonic(pkg, f0):
    """five-harmonic tones, 1 s at 16 kHz, through vits_tempo_host: the energy outside +-8 Hz of the harmonics at most -30 dB of the total (-33.6 dB at worst over the
    sixteen cases on the prototype of this definition, and on this implementation: 110 Hz at q = 2), the spectral peak within 0.5 Hz, the RMS within 1 %; the same
    overlap-add with every offset 0 (about 0 dB) must FAIL the -30 dB line, so a broken search cannot pass"""
    x = TR.harmonic_tone(f0)
    _, peak_in = TR.off_harmonic_db(x, f0)
    rms_in = np.sqrt((x[400:-400].astype(np.float64) ** 2).mean())
    for q in TONE_TEMPOS:
        q = float(np.float32(q))
        y, off = pkg.tempo_host(x, 16000, q)
        db, peak = TR.off_harmonic_db(y, f0)
        rms = np.sqrt((y[400:-400].astype(np.float64) ** 2).mean())
        y0, _ = TR.tempo(x, 16000, q, search=False)
        db0, _ = TR.off_harmonic_db(y0, f0)
        print(f"f0 = {f0} Hz, q = {q:.4f}: off-harmonic {db:.1f} dB (no search: {db0:.1f} dB), peak {peak:.3f} Hz (in: {peak_in:.3f}), RMS ratio {rms / rms_in:.5f}")
        assert db <= -30.0
        assert abs(peak - peak_in) <= 0.5
        assert abs(rms / rms_in - 1.0) <= 0.01
        assert db0 > -30.0
        assert off.any()


# ---- the plan table ----------------------------------------------------------------------------------------------------------------------------------
STAGES = ("vocoder", "tempo", "pitch", "edges", "level", "resample")
LEVELS = ("none", "measure", "gain", "whole")
ARENA = {"EDGE": "wave_edge", "LVL": "wave_lvl", "OUT": "wave_out", "PITCH": "wave_pitch", "TEMPO": "wave_tempo"}


def build(target):
    subprocess.check_call(["make", "-s", "-C", CSRC, target])
    return os.path.join(CSRC, target)


def test_tempo_plan_table_is_the_recorded_one():
    out = subprocess.run([build("delivery_plan_dump"), "tempo"], check=True, capture_output=True).stdout
    want = open(GOLDEN, "rb").read()
    if out != want:
        a, b = out.decode().splitlines(), want.decode().splitlines()
        diff = [(i + 1, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y][:10]
        raise AssertionError("tempo_plan_dump differs from the golden table (%d lines against %d); first differing lines (got, want):\n%s"
                             % (len(a), len(b), "\n".join("%d: %s\n   %s" % d for d in diff)))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
    got = subprocess.run([build("_asan/delivery_plan_dump"), "tempo"], capture_output=True, env=env)
    assert got.returncode == 0, got.stderr[-2000:]
    assert got.stdout == want


def test_host_definition_under_the_sanitizers():
    """tempo_host.cpp alone with its own main (tests/tempo_host_driver.cpp), built with -fsanitize=address,undefined and run as a program: buffers of exactly n, N'
    and F elements at four rates, eight tempos and twelve lengths each"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
    got = subprocess.run([build("_asan/tempo_host_driver")], capture_output=True, env=env)
    assert got.returncode == 0, got.stderr[-2000:]
    lines = got.stdout.decode().splitlines()
    assert len(lines) == 4 * 8 * 12
    for line in lines:
        rate, q, n, n_out, F = line.split()[:5]
        assert (int(F), int(n_out)) == TR.plan(int(rate), float(q), int(n))[3:], line


def rows():
    for line in open(GOLDEN).read().splitlines():
        key, fields = line.split(" : ", 1)
        ask = dict(kv.split("=") for kv in key.split())
        if fields.startswith("refuse "):
            yield ask, fields.split()[1], None, None, None
            continue
        parts = fields.split(" | ")
        assert len(parts) == 8 and [p.split()[0] for p in parts] == list(STAGES) + ["deliver", "needs"], line
        route = lambda r: tuple(r.split("/"))
        stages = {}
        for name, p in zip(STAGES, parts):
            what = p.split()[1]
            stages[name] = None if what == "off" else tuple(route(r) for r in what.split(">"))
        needs = parts[7].split()[1]
        yield ask, None, stages, route(parts[6].split()[1]), set() if needs == "-" else set(needs.split(","))


def test_the_tempo_table_covers_the_policy():
    R = list(rows())
    assert os.path.getsize(GOLDEN) < 128 * 1024
    keys = [tuple(a[k] for k in ("pitch", "edges", "level", "limiter", "rate", "out_device", "on_chunk", "async")) for a, *_ in R]
    want = [(p, e, lv) + rest for p in "01" for e in "01" for lv in LEVELS for rest in itertools.product("01", repeat=5)]
    assert keys == want and len(set(keys)) == len(keys) == 512
    # refused: every ask that streams, for the tempo first; with pitch, async as the pitch stage refuses it; with the edges stage, async as that stage does
    for ask, refusal, *_ in R:
        want_refusal = None
        if ask["on_chunk"] == "1":
            want_refusal = "tempo_stream"
        elif ask["async"] == "1" and ask["pitch"] == "1":
            want_refusal = "pitch_async"
        elif ask["async"] == "1" and ask["edges"] == "1":
            want_refusal = "edges_async"
        assert refusal == want_refusal, ask
    bufs = set()
    for ask, refusal, stages, delivered, needs in R:
        if refusal:
            continue
        od, pitch, edges = ask["out_device"] == "1", ask["pitch"] == "1", ask["edges"] == "1"
        assert stages["vocoder"] == (("NONE", "-"), ("WAVE", "S_stride")) and stages["tempo"] is not None
        assert (stages["pitch"] is not None) == pitch and (stages["edges"] is not None) == edges
        assert (stages["level"] is not None) == (ask["level"] != "none") and (stages["resample"] is not None) == (ask["rate"] == "1")
        # a chain in the order vocoder, tempo, pitch, edges, level, resample; the tempo stage reads the vocoder's rows, the pitch stage the tempo stage's
        cur = ("NONE", "-")
        writers = []
        for name in STAGES:
            if stages[name] is None:
                continue
            src, dst = stages[name]
            assert src == cur, (ask, name)
            if name == "level" and ask["level"] == "measure":
                assert dst == ("NONE", "-"), ask
                continue
            writers.append((name, dst))
            cur = dst
        assert delivered == cur, ask
        for name, dst in writers:
            assert (dst[0] == "CALLER") == (od and name == writers[-1][0]), (ask, name)
        assert stages["tempo"][0] == ("WAVE", "S_stride")
        if stages["tempo"][1][0] != "CALLER":
            assert stages["tempo"][1] == ("TEMPO", "T_stride")
        if pitch:
            assert stages["pitch"][0] == ("TEMPO", "T_stride")
            if stages["pitch"][1][0] != "CALLER":
                assert stages["pitch"][1] == ("PITCH", "P_stride")
        if edges:
            assert stages["edges"][0] == (("PITCH", "P_stride") if pitch else ("TEMPO", "T_stride"))
        # a levelled buffer follows its input's stride
        if stages["level"] and stages["level"][1][0] == "LVL":
            assert stages["level"][1][1] == ("E_stride" if edges else "P_stride" if pitch else "T_stride"), ask
        named = [r for st in stages.values() if st for r in st]
        bufs |= {b for b, _ in named}
        for buf, need in ARENA.items():
            assert (need in needs) == any(b == buf for b, _ in named), (ask, buf)
        assert ("ed_scratch" in needs) == edges and "join_table" not in needs and "wave_join" not in needs
        assert "out_ranges" not in needs and "lvl_ranges" not in needs
    assert bufs == {"NONE", "WAVE", "TEMPO", "PITCH", "EDGE", "LVL", "OUT", "CALLER"}
