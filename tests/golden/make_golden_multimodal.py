#!/usr/bin/env python3
"""Generate tests/golden/g7_sample_multimodal.npz by IMPORTING the reference's numpy half in place (same TensorFlow stub as
make_golden.py; nothing of the reference is copied, only the arrays its functions return).

Saved: the arrays of example_jbl/sample.jbl the multimodal model reads (feature, dense_adj, label, sequence,
sequence_length, sequence_symbol_num, max_node_num) and the `sequences` feed of kgcn/feed.py:178-181 for every batch of 10 over
the dataset in order (sample.jbl has 5 graphs, so one batch with five zero dummy rows), as construct_feed emits it.

    python tests/golden/make_golden_multimodal.py
"""
import contextlib
import io
import os

import joblib
import numpy as np

from make_golden import HERE, REF, _import_reference


def main():
    data_util, feed = _import_reference()
    raw = joblib.load(os.path.join(REF, "example_jbl", "sample.jbl"))
    cfg = {"with_feature": True, "with_node_embedding": False, "normalize_adj_flag": False, "split_adj_flag": False, "order": 1,
           "shuffle_data": False, "task": "classification"}
    with contextlib.redirect_stdout(io.StringIO()):
        all_data, info = data_util.load_data(cfg, os.path.join(REF, "example_jbl", "sample.jbl"), prohibit_shuffle=True)
    B = 10
    placeholders = {"sequences": "sequences", "mask": "mask"}
    batches, masks, idxs = [], [], []
    for it in range(0, all_data.num, B):
        idx = list(range(it, min(it + B, all_data.num)))
        fd = feed.construct_feed(idx, placeholders, all_data, batch_size=B, info=info, config=cfg)
        batches.append(fd["sequences"])
        masks.append(fd["mask"])
        idxs.append(np.asarray(idx + [-1] * (B - len(idx)), np.int64))
    np.savez_compressed(
        os.path.join(HERE, "g7_sample_multimodal.npz"),
        feature=np.asarray(raw["feature"], np.float64), dense_adj=np.asarray(raw["dense_adj"], np.int64),
        label=np.asarray(raw["label"], np.float64), sequence=np.asarray(raw["sequence"]),
        sequence_length=np.asarray(raw["sequence_length"], np.int64),
        sequence_symbol_num=np.int64(raw["sequence_symbol_num"]), max_node_num=np.int64(raw["max_node_num"]),
        info_sequence_symbol_num=np.int64(info.sequence_symbol_num), info_sequence_max_length=np.int64(info.sequence_max_length),
        feed_batch_size=np.int64(B), feed_batch_idx=np.stack(idxs), feed_sequences=np.stack(batches), feed_mask=np.stack(masks))


if __name__ == "__main__":
    main()
