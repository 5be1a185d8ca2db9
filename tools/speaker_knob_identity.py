"""Prints a hash of the PCM of fixed ragged batches with MIXED speakers on the FULL multi-speaker synthetic model; run under different
VITS_* knob settings: the hashes must be equal (the speaker-conditioned layers read the same effective-bias rows whichever kernel runs).
VITS_KNOB_ARITH = f32 | f16 | bf16. Batch 1 per speaker as well (the latency kernels: conv_lat16, the DDS head, conv16_lat pre, narrow flow)."""
import hashlib, os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from conftest import load_package
pkg = load_package()
m = pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL | pkg.SYNTH_SPEAKERS))
arith = {"f32": pkg.ARITH_F32, "f16": pkg.ARITH_F16, "bf16": pkg.ARITH_BF16}[os.environ.get("VITS_KNOB_ARITH", "f32")]
if arith != pkg.ARITH_F32:
    m.set_arith(arith)
ids = pkg.synth_ids(6, 48)
lens = np.array([48, 7, 33, 48, 1, 20], np.int32)
spk = np.array([2, -1, 0, 108, 2, 51], np.int32)
h = hashlib.sha256()
for mode in (0, 1):
    pcm, lengths, frames = m.process_batch(ids, id_lengths=lens, mode=mode, noise_seed=5, speaker_ids=spk)
    for p in pcm:
        h.update(p.tobytes())
for s in (-1, 0, 108):
    pcm, _, _ = m.process_batch(ids[:1], noise_seed=5, speaker_ids=[s])
    h.update(pcm[0].tobytes())
ids2 = pkg.synth_ids(40, 128, ids_seed=77)  # a wide grid: the throughput kernels (fused WaveNet layers, two flow chains, GEMM tiles)
pcm, _, _ = m.process_batch(ids2, noise_seed=6, speaker_ids=np.arange(40, dtype=np.int32) * 2 - 1)
for p in pcm:
    h.update(p.tobytes())
print(h.hexdigest()[:16])
