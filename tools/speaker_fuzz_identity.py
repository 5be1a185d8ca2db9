"""Randomised identity trials with mixed speakers (tests/fuzz_identity.py takes single-speaker models only): random ragged batches on
the FULL multi-speaker synthetic model, random speakers (-1 included), random semantics and arithmetic modes; every row must equal its
batch-1 call bit for bit (fp32; 16-bit modes too: every kernel is batch-invariant), and the windowed vocoder the whole one.
usage: python tools/speaker_fuzz_identity.py [--trials 40] [--seed 1]; prints one line per failure and a summary."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from conftest import load_package  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=40)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    pkg = load_package()
    rng = np.random.default_rng(a.seed)
    m = pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL | pkg.SYNTH_SPEAKERS))
    fails = 0
    for t in range(a.trials):
        B = int(rng.integers(1, 9))
        T = int(rng.integers(1, 160))
        lens = rng.integers(1, T + 1, size=B).astype(np.int32)
        ids = pkg.synth_ids(B, T, ids_seed=int(rng.integers(1, 1 << 30)))
        spk = rng.integers(-1, m.num_speakers, size=B).astype(np.int32)
        mode = int(rng.integers(0, 2))
        arith = [pkg.ARITH_F32, pkg.ARITH_F16, pkg.ARITH_BF16, pkg.ARITH_F32_SPLIT][int(rng.integers(0, 4))]
        seed = int(rng.integers(0, 1 << 20))
        m.set_arith(arith)
        pcm, lengths, frames = m.process_batch(ids, id_lengths=lens, mode=mode, noise_seed=seed, speaker_ids=spk)
        ok = True
        for b in range(B):
            one, _, f1 = m.process_batch(ids[b:b + 1, :lens[b]], mode=mode, noise_seed=seed, noise_seed_offsets=[b], speaker_ids=spk[b:b + 1])
            ok = ok and f1[0] == frames[b] and np.array_equal(one[0], pcm[b])
        win, _, _ = m.process_batch(ids, id_lengths=lens, mode=mode, noise_seed=seed, speaker_ids=spk, vocoder_chunk_frames=int(rng.integers(8, 80)))
        ok = ok and all(np.array_equal(x, y) for x, y in zip(win, pcm))
        if not ok:
            fails += 1
            print("FAIL trial", t, dict(B=B, T=T, lens=lens.tolist(), spk=spk.tolist(), mode=mode, arith=arith, seed=seed))
    m.close()
    print("speaker identity trials: %d, failures: %d" % (a.trials, fails))
    sys.exit(1 if fails else 0)


if __name__ == "__main__":
    main()
