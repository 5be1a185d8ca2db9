"""What the engine tests of the delivery stages (edges, level, limiter, output rate) share: bit comparison, the tiny model's ragged batch, the rule that
picks a trim threshold for the synthetic models, and a caller-owned device buffer.

The threshold. The synthetic models make stationary noise with no silence in it: the 10 ms windows of an utterance lie within a few dB of its loudest.
The tests therefore trim with TRIM_RELATIVE and a small drop: from the plain waveforms, the first threshold_db of CANDIDATES for which the restatement
(tests/edges_ref.py) moves a or b on at least `need` of the utterances with margin >= MARGIN on all of them; one must exist."""
import ctypes as C

import numpy as np

import edges_ref as ER

FS = 16000
LENS = np.array([5, 12, 31], np.int32)
MARGIN = 1e-6
CANDIDATES = (-0.5, -1.0, -1.5, -2.0, -3.0)
# keep margins shorter than a window (a trimmed window stays visible), fades and unequal pads
SHAPE = dict(keep_head_ms=2.5, keep_tail_ms=1.25, fade_in_ms=5.0, fade_out_ms=9.0, lead_ms=20.0, tail_ms=30.0)
PADS = 320 + 480


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def choose(waves, need=2):
    """the rule above: the first candidate that trims at least `need` of the utterances, with the margin on all of them"""
    for th in CANDIDATES:
        rows = [ER.edges(w, FS, ER.TRIM_RELATIVE, th, **SHAPE)[1] for w in waves]
        margins = [ER.margin(w, FS, ER.TRIM_RELATIVE, th, **SHAPE) for w in waves]
        trimmed = sum(int(r[0] > 0 or r[1] < w.size) for r, w in zip(rows, waves))
        print(f"threshold {th} dB: rows {[r.tolist() for r in rows]}, margins {['%.2e' % m for m in margins]}")
        if trimmed >= need and min(margins) >= MARGIN:
            return th
    return None


class DeviceRows:
    """a caller-owned float32 [rows][cols] device buffer (what out_device points at): fill(value), read() -> ndarray"""

    def __init__(self, rows, cols):
        self.shape = (rows, cols)
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.dev = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.dev), rows * cols * 4) == 0

    @property
    def ptr(self):
        return self.dev.value

    def fill(self, value):
        host = np.full(self.shape, value, np.float32)
        assert self.hip.hipMemcpy(self.dev, host.ctypes.data_as(C.c_void_p), host.nbytes, 1) == 0

    def read(self):
        got = np.zeros(self.shape, np.float32)
        assert self.hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), self.dev, got.nbytes, 2) == 0
        return got

    def __enter__(self):
        return self

    def __exit__(self, *a):
        if self.dev.value:
            self.hip.hipFree(self.dev)
            self.dev = C.c_void_p()
