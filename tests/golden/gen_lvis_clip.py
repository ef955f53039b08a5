"""Writes tests/golden/lvis_v1_clip.npy from the LVIS CLIP text matrix of the reference (`datasets/metadata/lvis_v1_clip_a+cname.npy`,
fp16 [1203, 512], 1.2 MB): every row scaled so that its largest magnitude is 127 and rounded to int8 (0.6 MB).

    python tests/golden/gen_lvis_clip.py <path to lvis_v1_clip_a+cname.npy>

The classifier normalises every class vector on load (NORM_WEIGHT), so the per-row scale drops out; what the rounding costs is
printed: cosine of every row with its original >= 0.9994, pairwise class cosines within 0.006 (mean 0.742 before and after).  The
fixture is for tests of vocabulary WIDTH and of the strongly correlated columns of real text embeddings, not for detection quality.
"""
import os
import sys

import numpy as np


def main(src: str) -> None:
    a = np.load(src).astype(np.float32)
    assert a.shape == (1203, 512), a.shape
    q = np.clip(np.rint(a / (np.abs(a).max(axis=1, keepdims=True) / 127.0)), -127, 127).astype(np.int8)
    an = a / np.linalg.norm(a, axis=1, keepdims=True)
    qn = q.astype(np.float32)
    qn /= np.linalg.norm(qn, axis=1, keepdims=True)
    off = ~np.eye(a.shape[0], dtype=bool)
    print(f"row cosine min {float((an * qn).sum(1).min()):.5f}; pairwise cosine max error {float(np.abs(an @ an.T - qn @ qn.T).max()):.4f}; "
          f"mean pairwise cosine {float((an @ an.T)[off].mean()):.4f} -> {float((qn @ qn.T)[off].mean()):.4f}")
    np.save(os.path.join(os.path.dirname(os.path.abspath(__file__)), "lvis_v1_clip.npy"), q)


if __name__ == "__main__":
    main(sys.argv[1])
