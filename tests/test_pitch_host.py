"""A stated pitch on the CPU (include/vits.h "a stated pitch"): the product's host-only pieces — vits_pitch_ratio, vits_pitch_plan, vits_pitch_table,
vits_pitch_host — against the float64 numpy restatement (tests/pitch_ref.py); what the definition does to sinusoids and how far its table lies from the
exact sinc, measured on the restatement; and the pitch half of the delivery planner against its frozen table.

tests/delivery_plan_dump.cpp (its slice `pitch`) links delivery_plan.o ALONE, walks every combination of the ask with pitch = true, joined or not, and prints one line per case; the
output must equal tests/golden/pitch_plan_table.txt byte for byte. The table was recorded once and is read line by line against the rules the last test
states; the test never regenerates it. The tables of the asks without pitch are tests/test_delivery_plan_host.py's and tests/test_joined_plan_host.py's,
which this stage leaves as they were."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import pitch_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vits.cpp_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "pitch_plan_table.txt")
RATIOS = (0.5, PR.ratio(-2), 1.0 - 2.0 ** -24, 1.0, 1.0 + 2.0 ** -23, PR.ratio(2), 1.5, 2.0)
FS = 16000


def test_ratio_and_plan_are_the_restatement(pkg):
    for st in (-12, -7, -2, -0.01, 0, 0.01, 2, 7, 12):
        assert pkg.pitch_ratio(st) == PR.ratio(st), st
    assert pkg.pitch_ratio(-12) == 0.5 and pkg.pitch_ratio(12) == 2.0 and pkg.pitch_ratio(0) == 1.0
    for p in RATIOS:
        for n in (0, 1, 2, 35, 71, 1000, 16001, 1 << 30):
            P, S, R, K, n_out = PR.plan(p, n)
            assert pkg.pitch_plan(p, n) == (P, S, R, n_out), (p, n)
    # the taps the definition states: 71 up to p = 1, 141 at p = 2
    assert PR.plan(0.5, 0)[3] == PR.plan(1.0, 0)[3] == 71 and PR.plan(2.0, 0)[3] == 141
    for bad in (float("nan"), float("inf"), float(np.nextafter(np.float32(0.5), np.float32(0))), float(np.nextafter(np.float32(2), np.float32(3))), 0.0, -1.0):
        with pytest.raises(pkg.VitsError, match=r"not finite or outside \[0.5, 2\]"):
            pkg.pitch_plan(bad, 10)
    for n in (-1, (1 << 30) + 1):
        with pytest.raises(pkg.VitsError, match=r"outside \[0, 2\^30\]"):
            pkg.pitch_plan(1.5, n)


def test_tables_are_the_definition(pkg):
    t = pkg.pitch_table()
    assert t.shape == (2, PR.ZQ + 2) and t.dtype == np.float32
    G, D = t
    assert np.abs(G.astype(np.float64) - PR.g0(np.arange(PR.ZQ + 2) / PR.Q)).max() <= 2.0 ** -24
    assert G[0] == 1.0 and G[PR.ZQ] == 0 and G[PR.ZQ + 1] == 0 and D[PR.ZQ + 1] == 0
    want = np.zeros_like(D)
    want[:-1] = G[1:] - G[:-1]  # (fp32 arithmetic)
    assert np.array_equal(D.view(np.uint32), want.view(np.uint32))


def test_host_evaluation_is_the_restatement(pkg):
    G, D = pkg.pitch_table()
    rng = np.random.default_rng(21)
    for p in RATIOS:
        R = PR.plan(p, 0)[2]
        for n in (1, 2, R, R + 1, 2 * R + 1, 257, 1000):
            x = rng.standard_normal(n).astype(np.float32)
            got = pkg.pitch_host(x, p)
            want, mag = PR.pitch(x, p, tables=(G, D), with_bound=True)
            assert got.size == want.size == PR.plan(p, n)[4]
            assert (np.abs(got - want) <= 1e-9 * mag).all(), (p, n)
    # (a row at ratio 1 goes through the filter in the host evaluation of the OTHER ratios only: at P = 2^24 the definition copies)
    x = rng.standard_normal(300).astype(np.float32)
    assert np.array_equal(PR.pitch(x, 1.0), x.astype(np.float64))


def peak_hz(y, fs):
    """the frequency of the largest spectral peak: Hann window, 8x zero padding, parabola through the log magnitudes around the largest bin"""
    n = 1 << int(np.ceil(np.log2(y.size)) + 3)
    m = np.abs(np.fft.rfft(y * np.hanning(y.size), n))
    k = int(m.argmax())
    a, b, c = np.log(m[k - 1:k + 2])
    return (k + 0.5 * (a - c) / (a - 2 * b + c)) * fs / n


@pytest.mark.parametrize("st", (-12, -7, -2, -0.01, 0.01, 2, 7, 12))
def test_a_tone_comes_out_at_its_shifted_frequency(st):
    p = PR.ratio(st)
    x = np.sin(2 * np.pi * 440.0 * np.arange(FS) / FS)
    y = PR.pitch(x, p)
    hz = peak_hz(y[200:-200], FS)
    print(f"{st:+} semitones: peak {hz:.4f} Hz, 440 p = {440 * p:.4f} Hz")
    assert abs(hz - 440.0 * p) <= 0.1


def level_db(p, hz):
    n = 6000
    x = np.sin(2 * np.pi * hz * np.arange(n) / FS)
    y = PR.pitch(x, p)[400:-400]  # (without the row's ends, where the tone is switched on and off)
    return 10 * np.log10((y ** 2).mean() / 0.5)


@pytest.mark.parametrize("p,hz", ((2.0, 4400.0), (2.0, 7000.0), (1.5, 6000.0), (PR.ratio(2), 7600.0)))
def test_tones_shifted_past_nyquist_are_stopped(p, hz):
    assert hz * p > FS / 2
    db = level_db(p, hz)
    print(f"p = {p}, {hz} Hz: {db:.1f} dB")
    assert db <= -90.0


@pytest.mark.parametrize("p,hz", ((2.0, 1000.0), (2.0, 3000.0), (1.5, 4000.0), (PR.ratio(2), 6000.0), (0.5, 7000.0), (PR.ratio(-2), 440.0)))
def test_tones_below_the_cutoff_pass(p, hz):
    assert hz * max(p, 1.0) < 0.92 * FS / 2
    db = level_db(p, hz)
    print(f"p = {p}, {hz} Hz: {db:.2f} dB")
    assert -1.0 <= db <= 0.05


def test_the_products_host_evaluation_shifts_and_stops_tones(pkg):
    """one tone and one stopband case of the two tests above through vits_pitch_host, with the same bounds: the product's own filter, not the restatement"""
    p = PR.ratio(2)
    y = pkg.pitch_host(np.sin(2 * np.pi * 440.0 * np.arange(FS) / FS).astype(np.float32), p)
    hz = peak_hz(y[200:-200], FS)
    print(f"+2 semitones through the product: peak {hz:.4f} Hz, 440 p = {440 * p:.4f} Hz")
    assert abs(hz - 440.0 * p) <= 0.1
    y = pkg.pitch_host(np.sin(2 * np.pi * 7000.0 * np.arange(6000) / FS).astype(np.float32), 2.0)[400:-400]
    db = 10 * np.log10((y ** 2).mean() / 0.5)
    print(f"p = 2, 7000 Hz through the product: {db:.1f} dB")
    assert db <= -90.0


@pytest.mark.parametrize("p", (0.5, 0.944, 1.059, 1.5, 2.0))
def test_the_table_is_close_to_the_exact_sinc(p):
    p = float(np.float32(p))
    x = np.random.default_rng(22).standard_normal(4000)
    exact = PR.pitch(x, p, exact=True)
    err = np.abs(PR.pitch(x, p) - exact).max() / np.sqrt((exact ** 2).mean())
    print(f"p = {p}: {err:.2e} of the output RMS")
    assert err <= 1e-4


# ---- the plan table ----------------------------------------------------------------------------------------------------------------------------------
STAGES = ("vocoder", "pitch", "edges", "join", "level", "resample")
LEVELS = ("none", "measure", "gain", "whole")
ARENA = {"EDGE": "wave_edge", "LVL": "wave_lvl", "OUT": "wave_out", "JOIN": "wave_join", "PITCH": "wave_pitch"}


def build(target):
    subprocess.check_call(["make", "-s", "-C", CSRC, target])
    return os.path.join(CSRC, target)


def test_pitch_plan_table_is_the_recorded_one():
    out = subprocess.run([build("delivery_plan_dump"), "pitch"], check=True, capture_output=True).stdout
    want = open(GOLDEN, "rb").read()
    if out != want:
        a, b = out.decode().splitlines(), want.decode().splitlines()
        diff = [(i + 1, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y][:10]
        raise AssertionError("pitch_plan_dump differs from the golden table (%d lines against %d); first differing lines (got, want):\n%s"
                             % (len(a), len(b), "\n".join("%d: %s\n   %s" % d for d in diff)))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
    got = subprocess.run([build("_asan/delivery_plan_dump"), "pitch"], capture_output=True, env=env)
    assert got.returncode == 0, got.stderr[-2000:]
    assert got.stdout == want


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


def test_the_pitch_table_covers_the_policy():
    R = list(rows())
    assert os.path.getsize(GOLDEN) < 128 * 1024
    keys = [tuple(a[k] for k in ("joined", "edges", "level", "limiter", "rate", "out_device", "on_chunk", "async")) for a, *_ in R]
    want = [(j, e, lv) + rest for j in "01" for e in "01" for lv in LEVELS for rest in itertools.product("01", repeat=5)]
    assert keys == want and len(set(keys)) == len(keys) == 512
    # refused: exactly the asks that stream or return early (a joined ask for being joined first, as ever)
    for ask, refusal, *_ in R:
        kind = "join" if ask["joined"] == "1" else "pitch"
        assert refusal == (kind + "_stream" if ask["on_chunk"] == "1" else kind + "_async" if ask["async"] == "1" else None), ask
    bufs, joined_seen = set(), 0
    for ask, refusal, stages, delivered, needs in R:
        if refusal:
            continue
        od, joined, edges = ask["out_device"] == "1", ask["joined"] == "1", ask["edges"] == "1"
        assert stages["vocoder"] == (("NONE", "-"), ("WAVE", "S_stride")) and stages["pitch"] is not None
        assert (stages["edges"] is not None) == edges and (stages["join"] is not None) == joined
        assert (stages["level"] is not None) == (ask["level"] != "none") and (stages["resample"] is not None) == (ask["rate"] == "1")
        # a chain in the order vocoder, pitch, edges, join, level, resample; the pitch stage reads the vocoder's rows
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
        # the stage's own rows are P_stride apart; the join variants route through it: the join reads the edges stage's rows, else the pitch stage's
        if stages["pitch"][1][0] != "CALLER":
            assert stages["pitch"][1] == ("PITCH", "P_stride")
        if edges:
            assert stages["edges"][0] == ("PITCH", "P_stride")
        if joined:
            joined_seen += 1
            assert stages["join"][0] == (("EDGE", "E_stride") if edges else ("PITCH", "P_stride")), ask
        # a levelled buffer follows its input's stride
        if stages["level"] and stages["level"][1][0] == "LVL":
            assert stages["level"][1][1] == ("J_stride" if joined else "E_stride" if edges else "P_stride"), ask
        named = [r for st in stages.values() if st for r in st]
        bufs |= {b for b, _ in named}
        for buf, need in ARENA.items():
            assert (need in needs) == any(b == buf for b, _ in named), (ask, buf)
        assert ("join_table" in needs) == joined and ("ed_scratch" in needs) == edges
        assert "out_ranges" not in needs and "lvl_ranges" not in needs
    assert joined_seen == 64 and bufs == {"NONE", "WAVE", "PITCH", "EDGE", "JOIN", "LVL", "OUT", "CALLER"}
