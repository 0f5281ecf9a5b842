"""Training sets of the vocabulary-trainer tests (tests/test_vocab_ref.py, tests/test_gpu_vocab_train.py): descriptors [n, 32]
uint8 and a CSR of images over them.  Deterministic; no GPU."""
from __future__ import annotations

import numpy as np

KL = [(10, 5), (2, 8), (8, 3), (32, 2)]


def offsets(n: int, n_images: int) -> np.ndarray:
    """n_images documents of (nearly) equal size; with n < n_images some are empty"""
    return np.linspace(0, n, n_images + 1).astype(np.int32)


def uniform(n: int, seed: int = 0) -> np.ndarray:
    return np.random.default_rng(0x70CAB + seed).integers(0, 256, (n, 32), dtype=np.uint8)


def clustered(n: int, seed: int = 0, noise: float = 0.04) -> np.ndarray:
    """leaves of synth.make_vocabulary, each bit flipped with probability `noise`"""
    from vo_slam_test_amd import synth
    voc = synth.make_vocabulary(seed, k=6, L=3)
    leaves = voc["node_desc"][voc["word_id"] >= 0]
    rng = np.random.default_rng(0xC1057 + seed)
    bits = np.unpackbits(leaves[rng.integers(0, len(leaves), n)], axis=1)
    bits ^= (rng.random(bits.shape) < noise).astype(np.uint8)
    return np.ascontiguousarray(np.packbits(bits, axis=1))


def duplicates(n: int, seed: int = 0, distinct: int = 37) -> np.ndarray:
    """n draws from `distinct` descriptors: many exact duplicates, far more descriptors than distinct values"""
    rng = np.random.default_rng(0xD0B1E + seed)
    base = rng.integers(0, 256, (distinct, 32), dtype=np.uint8)
    return np.ascontiguousarray(base[rng.integers(0, distinct, n)])


def all_equal(n: int, seed: int = 0) -> np.ndarray:
    one = np.random.default_rng(0xE90A1 + seed).integers(0, 256, 32, dtype=np.uint8)
    return np.ascontiguousarray(np.tile(one, (n, 1)))


def extracted(extract, n_frames: int = 6):
    """descriptors of synth frames, one image per frame.  extract(image) -> (key-points, descriptors): the device extractor
    (vo.OrbExtractor) on a GPU, the oracle's on a CPU -- the two are bit-identical (tests/test_gpu_orb.py)"""
    from vo_slam_test_amd import synth
    ds = [np.ascontiguousarray(extract(synth.make_frame(i))[1]) for i in range(n_frames)]
    off = np.concatenate([[0], np.cumsum([len(d) for d in ds])]).astype(np.int32)
    return np.ascontiguousarray(np.concatenate(ds)), off
