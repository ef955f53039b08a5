"""Writes tests/golden/lvis_v1_cat_freq.json from the LVIS v1 category statistics of the reference
(`datasets/metadata/lvis_v1_train_cat_info.json`): of every category only what `load_class_freq` reads, its id and its image count.

    python tests/golden/gen_lvis_cat_freq.py <path to lvis_v1_train_cat_info.json>

A file MODEL.ROI_BOX_HEAD.CAT_FREQ_PATH may name: the federated loss and IGNORE_ZERO_CATS tests train on it.
"""
import json
import os
import sys


def main(src: str) -> None:
    with open(src, "r") as fh:
        cats = json.load(fh)
    out = [{"id": int(c["id"]), "image_count": int(c["image_count"])} for c in sorted(cats, key=lambda c: c["id"])]
    assert len(out) == 1203 and [c["id"] for c in out] == list(range(1, 1204)), len(out)
    print(f"{len(out)} categories, image counts {min(c['image_count'] for c in out)} .. {max(c['image_count'] for c in out)}")
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "lvis_v1_cat_freq.json"), "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
        fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
