"""numpy restatement of trt_occluded's outputs (include/trt.h), for the tests: the documented mask layout, and "occluded"
read off a closest-hit record — ray i is occluded exactly when trt_trace reports id >= 0 for it."""
import numpy as np


def mask_words(n):
    return (int(n) + 63) // 64


def pack_mask(flags):
    """bool array (n,) -> (n + 63) // 64 uint64 words: bit i & 63 of word i >> 6 is ray i, the unused high bits zero."""
    f = np.asarray(flags).astype(bool).reshape(-1)
    padded = np.zeros(mask_words(len(f)) * 64, np.uint64)
    padded[:len(f)] = f
    return (padded.reshape(-1, 64) << np.arange(64, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)


def occluded_from_hits(hits):
    """hits: dict of SoA hit arrays (trt_trace / oracle.trace) -> bool array."""
    return np.asarray(hits["id"]) >= 0
