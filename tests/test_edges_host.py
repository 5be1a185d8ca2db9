"""The edges stage, host side (include/vits.h vits_model_set_edges): the plan integers, vits_edges_host against the float64 restatement
(tests/edges_ref.py) with the rows exact and y bit for bit on every signal in every mode, fades shorter and longer than the kept range, pads larger
than the row, the shortest rows, the defect each signal exposes, the refusals, the prototypes from C99, and the size of vits_process_opts. No device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import edges_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, W = ER.FS, 160
MARGIN = 1e-6
SIGNALS = ER.signals()
# fades shorter than anything kept, keep margins that are no multiple of a window, unequal pads
DESC = dict(keep_head_ms=12.5, keep_tail_ms=7.3, fade_in_ms=5.0, fade_out_ms=9.0, lead_ms=20.0, tail_ms=150.0)
MODES = ((ER.PAD, 0.0),) + ER.THRESHOLDS


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def check(pkg, x, fs, mode, threshold_db, **desc):
    """vits_edges_host against the restatement; returns (y, row)"""
    assert ER.margin(x, fs, mode, threshold_db, **desc) >= MARGIN
    want_y, want_row = ER.edges(x, fs, mode, threshold_db, **desc)
    y, row, tail = pkg.edges_host(x, fs, mode, threshold_db=threshold_db, **desc)
    assert np.array_equal(row, want_row), (row, want_row)
    assert same(y, want_y)
    p = ER.plan(fs, **desc)
    assert tail.size == x.size + p["Pl"] + p["Pt"] - row[2] and not tail.any() and not np.signbit(tail).any()  # [N', bound) is +0
    return y, row


@pytest.mark.parametrize("fs,W_,tile", [(8000, 80, 4080), (11025, 110, 4070), (16000, 160, 4000), (22050, 221, 3978), (44100, 441, 3969), (48000, 480, 3840)])
def test_plan_integers(pkg, fs, W_, tile):
    got = pkg.edges_plan(fs, pkg.EDGES_TRIM_RELATIVE, threshold_db=-40.0, **DESC)
    p = ER.plan(fs, **DESC)
    assert got[:7] == (W_, p["Kh"], p["Kt"], p["Fi"], p["Fo"], p["Pl"], p["Pt"])
    assert W_ == (fs + 50) // 100
    # samples(ms) = floor(ms fs / 1000 + 0.5) of the fp32 field: 12.5 ms, 7.3 ms (7.30000019 as fp32), 5, 9, 20, 150 ms
    want = {8000: (100, 58, 40, 72, 160, 1200), 11025: (138, 80, 55, 99, 221, 1654), 16000: (200, 117, 80, 144, 320, 2400),
            22050: (276, 161, 110, 198, 441, 3308), 44100: (551, 322, 221, 397, 882, 6615), 48000: (600, 350, 240, 432, 960, 7200)}[fs]
    assert got[1:7] == want
    assert got[7] == tile and tile % W_ == 0 and tile <= 4096 < tile + W_  # the window kernel's tile: the largest multiple of W at or under 4096
    # a half rounds up: 0.03125 ms at 16 kHz is exactly half a sample
    assert pkg.edges_plan(16000, pkg.EDGES_PAD, lead_ms=0.03125)[5] == 1 and pkg.edges_plan(16000, pkg.EDGES_PAD, lead_ms=0.03)[5] == 0
    assert (pkg.EDGES_OFF, pkg.EDGES_PAD, pkg.EDGES_TRIM_RELATIVE, pkg.EDGES_TRIM_ABSOLUTE) == (0, 1, 2, 3) == (ER.OFF, ER.PAD, ER.TRIM_RELATIVE, ER.TRIM_ABSOLUTE)


@pytest.mark.parametrize("mode,threshold_db", MODES)
@pytest.mark.parametrize("name", sorted(SIGNALS))
def test_host_equals_the_restatement(pkg, name, mode, threshold_db):
    x = SIGNALS[name]
    y, row = check(pkg, x, FS, mode, threshold_db, **DESC)
    a, b, n1, n_active = (int(v) for v in row)
    if mode == ER.PAD:
        assert (a, b, n_active) == (0, x.size, 0) and n1 == x.size + 320 + 2400
        return
    want = {  # (a, b, n_active) under either threshold: Kh = 200, Kt = 117
        "onset_edge": (5 * W - 200, 9 * W + 117, 4), "onset_before": (4 * W - 200, 10 * W + 117, 6), "onset_after": (5 * W - 200, 9 * W + 117, 4),
        "partial_last": (4000 - 200, 4007, 1), "silent_zeros": (0, 0, 0), "all_active": (0, x.size, 26), "single": (7 * W - 200, 8 * W + 117, 1),
        "ends_at_n": (6 * W - 200, x.size, 20),
        # a floor alone: every window is within a few dB of the loudest (RELATIVE keeps all of it), and 15 dB under the absolute threshold
        "silent_floor": (0, x.size, 26) if mode == ER.TRIM_RELATIVE else (0, 0, 0),
    }[name]
    assert (a, b, n_active) == want and n1 == 320 + (b - a) + 2400


def test_fades_longer_than_the_kept_range_overlap_and_pads_larger_than_the_row(pkg):
    x = SIGNALS["single"]
    # one active window and no keep margin: M = 160 under fades of 400 and 640 samples and pads of 1.5 N
    desc = dict(fade_in_ms=25.0, fade_out_ms=40.0, lead_ms=375.0, tail_ms=380.0)
    for mode, th in MODES:
        y, row = check(pkg, x, FS, mode, th, **desc)
        assert row[2] == 6000 + 6080 + (x.size if mode == ER.PAD else W)
    y, row = check(pkg, x, FS, ER.TRIM_RELATIVE, -35.0, **desc)
    mid = y[6000:6000 + W]
    win, wout = ER.fade(400), ER.fade(640)
    assert same(mid, (x[7 * W:8 * W] * win[:W]) * wout[:W][::-1])  # nothing is rescaled: both tables apply to every sample
    assert np.abs(mid).max() < 0.1 * float(win[W - 1])
    # fades of exactly M, of M - 1 and of M + 1
    for F in (W - 1, W, W + 1):
        check(pkg, x, FS, ER.TRIM_ABSOLUTE, -55.0, fade_in_ms=F / 16.0, fade_out_ms=F / 16.0)


@pytest.mark.parametrize("n", (0, 1, W - 1, W, W + 1))
def test_the_shortest_rows(pkg, n):
    x = ER.burst(np.zeros(n, np.float32), 0, n, seed=90 + n % 7)
    for mode, th in MODES:
        for desc in (DESC, dict(fade_in_ms=1.0, fade_out_ms=1.0), {}):
            y, row = check(pkg, x, FS, mode, th, **desc)
            p = ER.plan(FS, **desc)
            assert row[0] == 0 and row[1] == n and row[2] == n + p["Pl"] + p["Pt"]
            assert row[3] == (0 if mode == ER.PAD else -(-n // W))
    # a row nothing touches is x bit for bit
    y, row = check(pkg, x, FS, ER.TRIM_RELATIVE, -35.0)
    assert same(y, x)


def test_nans_are_inactive_windows_and_a_relative_threshold_ignores_them(pkg):
    x = SIGNALS["single"].copy()
    x[2 * W + 5] = np.nan  # q of window 2 is a NaN: it compares false, and q_max is the largest q that is not a NaN
    for mode, th in ER.THRESHOLDS:
        want_y, want_row = ER.edges(x, FS, mode, th, **DESC)
        y, row, _ = pkg.edges_host(x, FS, mode, threshold_db=th, **DESC)
        assert np.array_equal(row, want_row) and same(y, want_y) and tuple(row[:2]) == (7 * W - 200, 8 * W + 117) and row[3] == 1


@pytest.mark.parametrize("defect,name,mode,threshold_db,desc", [
    ("keep", "onset_edge", ER.TRIM_RELATIVE, -35.0, DESC),       # a dropped keep margin: a and b move by Kh and Kt
    ("partial", "partial_last", ER.TRIM_ABSOLUTE, -55.0, DESC),  # a dropped partial window: the only burst is lost, nothing is delivered
    ("partial", "ends_at_n", ER.TRIM_RELATIVE, -35.0, dict(DESC, keep_tail_ms=1.0)),  # ... or b stops short of N (a keep margin of 16 samples hides 16 of the 33)
    ("strict", "single", ER.TRIM_RELATIVE, 0.0, DESC),           # > in place of >= at q_max: the loudest window is not active
    # a fade indexed from the wrong end: the head is faded twice, the tail not at all (no keep margin behind: the last kept sample is a burst sample)
    ("fade_end", "onset_edge", ER.TRIM_RELATIVE, -35.0, dict(DESC, keep_tail_ms=0.0)),
])
def test_each_signal_exposes_its_defect(pkg, defect, name, mode, threshold_db, desc):
    x = SIGNALS[name]
    y, row = check(pkg, x, FS, mode, threshold_db, **desc)
    bad_y, bad_row = ER.edges(x, FS, mode, threshold_db, defect=defect, **desc)
    assert not np.array_equal(row, bad_row) or not same(y, bad_y)
    if defect == "keep":
        assert (bad_row[0], bad_row[1]) == (row[0] + 200, row[1] - 117)
    elif defect == "partial":
        assert bad_row[3] == row[3] - 1 and bad_row[1] < row[1]
    elif defect == "strict":
        assert row[3] == 1 and bad_row[3] == 0 and bad_row[2] == 320 + 2400
    else:
        assert np.array_equal(row, bad_row) and not same(y[-2400 - 144:-2400], bad_y[-2400 - 144:-2400])
        assert np.abs(y[-2401]) < 1e-3 * 0.1 < 0.09 < np.abs(bad_y[-2401])  # the last kept sample: faded out, or left at full level


def test_refusals(pkg):
    x = np.zeros(8, np.float32)
    for field in ER.FIELDS:
        for bad in (-0.5, 2000.5, float("nan"), float("inf")):
            for call in (lambda **k: pkg.edges_plan(FS, pkg.EDGES_PAD, **k), lambda **k: pkg.edges_host(x, FS, pkg.EDGES_PAD, **k)):
                with pytest.raises(pkg.VitsError, match=field):
                    call(**{field: bad})
    for bad in (0.5, -120.5, float("nan")):
        for mode in (pkg.EDGES_TRIM_RELATIVE, pkg.EDGES_TRIM_ABSOLUTE):
            with pytest.raises(pkg.VitsError, match="threshold_db"):
                pkg.edges_plan(FS, mode, threshold_db=bad)
        pkg.edges_plan(FS, pkg.EDGES_PAD, threshold_db=bad)  # ignored by PAD
    for mode in (-1, 4, 9):
        with pytest.raises(pkg.VitsError, match="unknown mode"):
            pkg.edges_plan(FS, mode)
    for fs in (3999, 192001):
        with pytest.raises(pkg.VitsError, match=str(fs)):
            pkg.edges_plan(fs, pkg.EDGES_PAD)
        with pytest.raises(pkg.VitsError, match=str(fs)):
            pkg.edges_host(x, fs, pkg.EDGES_PAD)
    pkg.edges_plan(192000, pkg.EDGES_PAD, lead_ms=2000.0)
    with pytest.raises(pkg.VitsError, match="VITS_EDGES_OFF"):
        pkg.edges_host(x, FS, pkg.EDGES_OFF)
    L = pkg.lib()
    d = pkg.edges_desc(pkg.EDGES_PAD, lead_ms=1.0)
    out, row, y = np.zeros(8, np.int64), np.zeros(4, np.int64), np.zeros(64, np.float32)
    for size in (0, 32, 40):
        d.struct_size = size
        assert L.vits_edges_plan(FS, C.byref(d), out.ctypes.data) == -1 and "struct_size" in pkg.last_error()
        assert L.vits_edges_host(x.ctypes.data, 8, FS, C.byref(d), y.ctypes.data, 64, row.ctypes.data) == -1 and "struct_size" in pkg.last_error()
    d.struct_size = C.sizeof(pkg.EdgesDesc)
    assert C.sizeof(pkg.EdgesDesc) == 36
    assert L.vits_edges_plan(FS, None, out.ctypes.data) == -1 and "null" in pkg.last_error()
    assert L.vits_edges_plan(FS, C.byref(d), None) == 0
    assert L.vits_edges_host(None, 4, FS, C.byref(d), None, 0, None) == -1 and "null" in pkg.last_error()
    assert L.vits_edges_host(None, 0, FS, C.byref(d), None, 0, row.ctypes.data) == 0 and list(row) == [0, 0, 16, 0]  # (an empty row: the pads alone)
    assert L.vits_edges_host(x.ctypes.data, 8, FS, C.byref(d), y.ctypes.data, 8 + 16 - 1, row.ctypes.data) == -1 and "y_cap" in pkg.last_error()
    assert L.vits_edges_host(x.ctypes.data, 8, FS, C.byref(d), y.ctypes.data, 8 + 16, row.ctypes.data) == 0
    # the handle-level entry points refuse a NULL model without touching it
    assert L.vits_model_set_edges(None, C.byref(d)) == -1 and L.vits_model_get_edges(None, C.byref(d)) == -1 and L.vits_model_last_edges(None, None, 0) == -1
    for name in ("vits_model_set_edges", "vits_model_get_edges", "vits_model_last_edges", "vits_edges_plan", "vits_edges_host", "vits_op_edges"):
        assert hasattr(L, name) and name in pkg.EXPORTED_SYMBOLS


def test_a_c99_caller_links_and_process_opts_keeps_its_size(pkg, tmp_path):
    src = tmp_path / "edges.c"
    src.write_text('#include <stdio.h>\n#include <string.h>\n#include "vits.h"\n'
                   'int main(void) {\n'
                   '  int (*a)(vits_model*, const vits_edges_desc*) = vits_model_set_edges;\n'
                   '  int (*b)(const vits_model*, vits_edges_desc*) = vits_model_get_edges;\n'
                   '  int64_t (*c)(vits_model*, int64_t*, size_t) = vits_model_last_edges;\n'
                   '  int (*d)(int32_t, const vits_edges_desc*, int64_t*) = vits_edges_plan;\n'
                   '  int (*e)(const float*, size_t, int32_t, const vits_edges_desc*, float*, size_t, int64_t*) = vits_edges_host;\n'
                   '  int (*f)(int32_t, const vits_edges_desc*, int32_t, const float*, int64_t, const int32_t*, float*, int64_t, int32_t*, int64_t*) = vits_op_edges;\n'
                   '  vits_edges_desc k; int64_t out[8], row[4]; float x[4] = {0.5f, -0.5f, 0.25f, 0.0f}, y[8];\n'
                   '  memset(&k, 0, sizeof k); k.struct_size = sizeof k; k.mode = VITS_EDGES_PAD; k.lead_ms = 0.125f; k.tail_ms = 0.125f;\n'
                   '  int ok = d(16000, &k, out) == 0 && out[0] == 160 && out[5] == 2 && e(x, 4, 16000, &k, y, 8, row) == 0 && row[2] == 8 && y[2] == 0.5f && y[7] == 0.0f;\n'
                   '  int refused = a(NULL, &k) == -1 && b(NULL, &k) == -1 && c(NULL, NULL, 0) == -1 && f(16000, &k, 0, x, 4, NULL, y, 8, NULL, row) == -1;\n'
                   '  printf("%zu %zu %d %d %d\\n", sizeof(vits_process_opts), sizeof(vits_edges_desc), ok, refused, VITS_EDGES_TRIM_ABSOLUTE); return 0; }\n')
    exe = tmp_path / "edges"
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", lib_dir, "-lvits_hip",
                    "-Wl,-rpath," + lib_dir], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["160", "36", "1", "1", "3"]
    assert C.sizeof(pkg.ProcessOpts) == 160
