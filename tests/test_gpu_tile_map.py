"""Ragged batches on the lists of existing tiles (tile_map.h), whole model: the PCM and the lengths under VITS_TILE_MAP=1 (a list wherever a converted kernel
runs) are those of VITS_NO_TILE_MAP=1 (dense grids everywhere), bit for bit.

A ragged batch of five utterances of 2 ... 24 ids through the full synthetic model: both semantics modes, a windowed vocoder whose later windows hold no
frames of the shorter utterances (their lists are empty there), the per-kernel profiler's schedule (the grouped launch of the wide stages), and the
submit_batch / wait pipeline (its lists travel through the slot's pinned memory). At these sizes the planner would give the convolutions its small tiles,
which keep their dense grids; VITS_MIN_BLOCKS=1, VITS_NO_LAT16 and VITS_NO_NARROW (both runs alike) keep them on the 128 x 128 tile that runs the lists."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TS = [24, 2, 17, 9, 5]


HALO = 17  # the vocoder's receptive field in frames, one side, for this architecture (engine_load.cpp): window w computes frames [f0 - HALO, f1 + HALO)


def run_all(pkg, full_bytes):
    ids = pkg.synth_ids(5, 24)
    ref, hf = pkg.MODE_REFERENCE, pkg.MODE_HF
    out = {}
    n0 = pkg.op_tile_map_launches()
    with pkg.Model(full_bytes) as m:
        out["plain", ref] = m.process_batch(ids, id_lengths=TS, mode=ref, noise_seed=9)
        frames = out["plain", ref][2]
        chunk = max(4, (int(frames.max()) - 1) // 3)  # four windows or so; the last ones start behind the short utterances' ends
        last_f0 = chunk * ((int(frames.max()) - 1) // chunk)
        assert frames.min() <= last_f0 - HALO, (frames, chunk)  # an utterance without a frame in the last window: its lists are empty there
        out["plain", hf] = m.process_batch(ids, id_lengths=TS, mode=hf, noise_seed=9)
        for mode in (ref, hf):
            out["windowed", mode] = m.process_batch(ids, id_lengths=TS, mode=mode, noise_seed=9, vocoder_chunk_frames=chunk)
        m.prof_enable(True)
        out["profiler"] = m.process_batch(ids, id_lengths=TS, mode=ref, noise_seed=9)
        names = [k["name"] for k in m.prof_report()["kernels"]]
        assert any("hifigan_resblock_group" in n for n in names), names
        m.prof_enable(False)
        m.submit_batch(ids, id_lengths=TS, mode=ref, noise_seed=9)
        m.submit_batch(ids, id_lengths=TS, mode=ref, noise_seed=9, vocoder_chunk_frames=chunk)
        out["pipelined"] = m.wait()
        out["pipelined_windowed"] = m.wait()
    return out, pkg.op_tile_map_launches() - n0


def test_lists_give_the_bits_of_the_dense_grids(pkg, full_bytes, monkeypatch):
    for knob in ("VITS_MIN_BLOCKS", "VITS_NO_LAT16", "VITS_NO_NARROW"):
        monkeypatch.setenv(knob, "1")
    monkeypatch.delenv("VITS_TILE_MAP", raising=False)
    monkeypatch.setenv("VITS_NO_TILE_MAP", "1")
    dense, n_dense = run_all(pkg, full_bytes)
    monkeypatch.delenv("VITS_NO_TILE_MAP")
    monkeypatch.setenv("VITS_TILE_MAP", "1")
    listed, n_listed = run_all(pkg, full_bytes)
    assert n_dense == 0 and n_listed > 0, (n_dense, n_listed)
    assert dense.keys() == listed.keys()
    for key in dense:
        (pa, la, fa), (pb, lb, fb) = dense[key], listed[key]
        assert np.array_equal(la, lb) and np.array_equal(fa, fb), key
        for u, (x, y) in enumerate(zip(pa, pb)):
            assert x.size == la[u] and np.array_equal(x.view(np.uint32), y.view(np.uint32)), (key, u)
    # the windowed and the pipelined runs are the plain run again (so the lists of every window and of the slot's pinned copy were the right ones)
    for key, ref in (("windowed", "plain"),):
        for mode in (pkg.MODE_REFERENCE, pkg.MODE_HF):
            for x, y in zip(listed[key, mode][0], listed[ref, mode][0]):
                assert np.array_equal(x, y), (key, mode)
    for key in ("profiler", "pipelined", "pipelined_windowed"):
        for x, y in zip(listed[key][0], listed["plain", pkg.MODE_REFERENCE][0]):
            assert np.array_equal(x, y), key
