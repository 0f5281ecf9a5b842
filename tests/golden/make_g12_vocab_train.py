"""Regenerates tests/golden/g12_vocab_train.npz: one training set (4000 descriptors, 16 images) and the tree the numpy
restatement of the DESIGN.md §4d contract (tests/vocab_ref.py) builds from it with k = 5, L = 3.  Pins the restatement
against its own drift.  Run from the repository root: python tests/golden/make_g12_vocab_train.py"""
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import vocab_inputs as I  # noqa: E402
import vocab_ref as R  # noqa: E402

n, k, L, seed = 4000, 5, 3, 12
desc = np.concatenate([I.clustered(3000, seed=12), I.uniform(1000, seed=12)])
off = I.offsets(n, 16)
t = R.train(desc, off, k, L, seed)
info = np.array([t["info"][x] for x in ("n_nodes", "n_words", "n_levels", "lloyd_iterations_max", "n_capped")], np.int32)
out = ROOT / "tests" / "golden" / "g12_vocab_train.npz"
np.savez_compressed(out, desc=desc, image_offsets=off, k=k, L=L, seed=seed, child_start=t["child_start"], children=t["children"],
                    node_desc=t["node_desc"], word_id=t["word_id"], node_weight=t["node_weight"], info=info)
print(out, out.stat().st_size, "bytes", t["info"])
